// The product's partition routines (csrc/dxv_partition.h, through tests/hostcheck/partition_check.cpp) in a program of their own, for a build
// with -fsanitize=address,undefined: sides 2, 6, 18 and 34, a seeded union of balls and a dense random grid, both kinds, caps 1, 5 and 101, every
// value of partprune, the centres forwards, backwards and shuffled, with and without throats.  Every run of a grid must give the same labels,
// table and throats as its first.  Prints one line per grid, cap and kind; exits 0 when everything agrees.
#include "../hostcheck/partition_check.cpp"

#include <cstdio>

static uint32_t g_state = 12345u;
static uint32_t next() { return g_state = g_state * 1664525u + 1013904223u; }

static std::vector<uint8_t> make_grid(uint32_t N, int what)
{
    std::vector<uint8_t> g((size_t)N * N * N, 0);
    if (what == 0) {
        for (int b = 0; b < 6; ++b) {
            const int cx = (int)(next() % N), cy = (int)(next() % N), cz = (int)(next() % N), r = 1 + (int)(next() % (N / 3u + 1u));
            for (int z = 0; z < (int)N; ++z)
                for (int y = 0; y < (int)N; ++y)
                    for (int x = 0; x < (int)N; ++x)
                        if ((x - cx) * (x - cx) + (y - cy) * (y - cy) + (z - cz) * (z - cz) <= r * r) g[((size_t)z * N + y) * N + x] = 0x80;
        }
    } else {
        for (uint8_t& v : g) v = (next() >> 16) % 10u < 6u ? 1 : 0;
    }
    return g;
}

static bool same_bytes(const void* a, const void* b, size_t n) { return !n || !memcmp(a, b, n); }

int main()
{
    const uint32_t sides[] = {2u, 6u, 18u, 34u}, caps[] = {1u, 5u, 101u};
    for (uint32_t N : sides)
        for (int what = 0; what < 2; ++what) {
            const std::vector<uint8_t> g = make_grid(N, what);
            for (uint32_t cap : caps)
                for (int of = 0; of < 2; ++of) {
                    std::vector<uint32_t> labels;
                    std::vector<PartRegion> table;
                    std::vector<PartThroat> throats;
                    uint64_t first[5] = {};
                    for (uint32_t prune = 0; prune < 4u; ++prune)
                        for (int order = 0; order < 3; ++order) {
                            uint64_t counts[5] = {};
                            if (pc_partition(g.data(), N, of, cap, prune, order, 1, counts)) { fprintf(stderr, "refused\n"); return 1; }
                            if (!prune && !order) { labels = g_labels; table = g_table; throats = g_throats; memcpy(first, counts, sizeof first); continue; }
                            if (counts[0] != first[0] || counts[1] != first[1] || counts[2] != first[2] || g_labels != labels ||
                                !same_bytes(g_table.data(), table.data(), table.size() * sizeof(PartRegion)) ||
                                !same_bytes(g_throats.data(), throats.data(), throats.size() * sizeof(PartThroat)))
                            { fprintf(stderr, "N %u cap %u of %d: partprune %u order %d differs\n", N, cap, of, prune, order); return 1; }
                        }
                    uint64_t counts[5] = {}, voxels = 0;
                    if (pc_partition(g.data(), N, of, cap, 3u, 0, 0, counts)) return 1;
                    for (const PartRegion& r : g_table) { voxels += r.voxels; if (r.throats) { fprintf(stderr, "a throat count without throats\n"); return 1; } }
                    if (g_labels != labels || counts[1] || counts[2] || !g_throats.empty()) { fprintf(stderr, "N %u cap %u of %d: without throats differs\n", N, cap, of); return 1; }
                    uint64_t members = 0;
                    for (uint32_t l : labels) members += l != 0u;
                    if (voxels != members) { fprintf(stderr, "the regions hold %llu of %llu members\n", (unsigned long long)voxels, (unsigned long long)members); return 1; }
                    printf("N %u grid %d cap %u of %d: %llu regions, %llu throats, %llu faces\n", N, what, cap, of, (unsigned long long)first[0], (unsigned long long)first[1],
                           (unsigned long long)first[2]);
                }
        }
    return 0;
}
