// The product's access routines (csrc/dxv_access.h, through tests/hostcheck/access_check.cpp) in a program of their own, for a build with
// -fsanitize=address,undefined.  The grids: the builders' (tests/access_restated.py: the ink bottles, the chamber raised twice, the staircase,
// the checkerboard, a random grid, the hollow box), which the test writes into the file named on the command line -- per grid the side, the
// number of listed seeds, the seeds, N^3 bytes --; and, for what the builders' sides do not reach, sparse and dense random grids at sides 2, 6,
// 10 and 26: a side below a tile, partial tiles, a halo outside the grid on every side.  Every grid runs for both kinds, both connectivities
// and the three kinds of seeds, with the intrusion map, every round's tiles in index order and shuffled.  The two orders must give the same
// maps, A must not exceed the map of every member seeded, I must not be below A, and the tally must count every member once.  Prints one line
// per run; exits 0 when everything agrees.
#include "../hostcheck/access_check.cpp"

#include <cstdio>

static uint32_t g_state = 2463534242u;
static uint32_t next() { return g_state = g_state * 1664525u + 1013904223u; }

static int run_grid(const char* what, uint32_t N, const std::vector<uint8_t>& g, const std::vector<uint32_t>& list, uint32_t cap)
{
    const uint32_t n3 = N * N * N;
    std::vector<uint8_t> mask(n3), all(n3, 1);
    for (uint8_t& v : mask) v = next() % 97u == 0u ? 0x40 : 0;
    for (int of = 0; of < 2; ++of)
        for (int connectivity = 6; connectivity <= 26; connectivity += 20)
            for (int kind = 0; kind < 3; ++kind) {
                const void* seeds = kind == GEO_SEEDS_LIST ? (const void*)list.data() : kind == GEO_SEEDS_MASK ? (const void*)mask.data() : nullptr;
                const uint32_t count = kind == GEO_SEEDS_LIST ? (uint32_t)list.size() : 0u;
                std::vector<uint32_t> A(n3), I(n3), A2(n3), I2(n3), R(n3);
                std::vector<uint64_t> histA(cap + 1u), histI(cap + 1u), h2(cap + 1u), h3(cap + 1u);
                uint64_t tally[5], shuffled[5], every[5], work[2];
                if (ac_access(g.data(), N, of, connectivity, cap, kind, seeds, count, 3u, 0u, A.data(), I.data(), histA.data(), histI.data(), tally, work)) { fprintf(stderr, "refused\n"); return 1; }
                if (ac_access(g.data(), N, of, connectivity, cap, kind, seeds, count, 0u, N + (uint32_t)kind + 1u, A2.data(), I2.data(), h2.data(), h3.data(), shuffled, work)) { fprintf(stderr, "refused\n"); return 1; }
                if (ac_access(g.data(), N, of, connectivity, cap, GEO_SEEDS_MASK, all.data(), 0u, 3u, 0u, R.data(), nullptr, h2.data(), h3.data(), every, work)) { fprintf(stderr, "refused\n"); return 1; }
                uint64_t members = 0;
                for (uint32_t v = 0; v < n3; ++v) {
                    members += geo_member(g[v], of) ? 1u : 0u;
                    if (A[v] != A2[v] || I[v] != I2[v] || A[v] > R[v] || I[v] < A[v] || (R[v] != 0u) != geo_member(g[v], of)) { fprintf(stderr, "%s N %u: voxel %u\n", what, N, v); return 1; }
                }
                if (tally[1] + tally[2] != members || every[0] != members || every[1] != members) { fprintf(stderr, "%s N %u: the tally counts %llu of %llu members\n", what, N, (unsigned long long)(tally[1] + tally[2]), (unsigned long long)members); return 1; }
                for (int k = 0; k < 5; ++k)
                    if (tally[k] != shuffled[k]) return 1;
                if (!tally[1] && (tally[4] != 0xFFFFFFFFu || tally[3] != 0u)) return 1;
                printf("%s N %u cap %u of %d connectivity %d seeds %d: used %llu reached %llu unreached %llu widest %llu at %llu\n", what, N, cap, of, connectivity, kind,
                       (unsigned long long)tally[0], (unsigned long long)tally[1], (unsigned long long)tally[2], (unsigned long long)tally[3], (unsigned long long)tally[4]);
            }
    return 0;
}

int main(int argc, char** argv)
{
    if (argc != 2) { fprintf(stderr, "usage: %s builders.bin\n", argv[0]); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
    uint32_t head[2], builders = 0;
    while (fread(head, sizeof(uint32_t), 2, f) == 2) {
        const uint32_t N = head[0];
        if (N < 2u || N > 64u || head[1] > 64u) { fprintf(stderr, "a builder of side %u with %u seeds\n", N, head[1]); return 2; }
        std::vector<uint32_t> list(head[1]);
        std::vector<uint8_t> g((size_t)N * N * N);
        if (fread(list.data(), sizeof(uint32_t), list.size(), f) != list.size() || fread(g.data(), 1, g.size(), f) != g.size()) { fprintf(stderr, "a short builder\n"); return 2; }
        if (run_grid("builder", N, g, list, (builders & 1u) ? 65u : 4096u)) return 1;
        ++builders;
    }
    fclose(f);
    if (!builders) { fprintf(stderr, "no builder in %s\n", argv[1]); return 2; }
    const uint32_t sides[] = {2u, 6u, 10u, 26u};
    for (uint32_t N : sides)
        for (uint32_t density = 3; density <= 7u; density += 4u) {
            const uint32_t n3 = N * N * N;
            std::vector<uint8_t> g(n3);
            for (uint8_t& v : g) v = next() % 10u < density ? (uint8_t)(1u + next() % 255u) : 0;
            std::vector<uint32_t> list;
            for (uint32_t k = 0; k < 5u; ++k) list.push_back(next() % n3);
            list.push_back(list[0]);                                    // a duplicate
            if (run_grid(density == 3u ? "sparse" : "dense", N, g, list, density == 3u ? 65u : 4096u)) return 1;
        }
    uint64_t tally[5], work[2];
    std::vector<uint8_t> g(8, 1);
    std::vector<uint32_t> A(8), I(8);
    std::vector<uint64_t> h(66), hi(66);
    const uint32_t outside[] = {3u, 8u};
    if (ac_access(g.data(), 2, 0, 6, 65, GEO_SEEDS_LIST, outside, 2u, 3u, 0u, A.data(), I.data(), h.data(), hi.data(), tally, work) != 1) { fprintf(stderr, "an index outside the grid accepted\n"); return 1; }
    return 0;
}
