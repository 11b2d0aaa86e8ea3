// The product's geodesic routines (csrc/dxv_geodesic.h, through tests/hostcheck/geodesic_check.cpp) in a program of their own, for a build with
// -fsanitize=address,undefined: sides 1, 2, 7, 9, 16 and 27 -- partial tiles, a halo outside the grid on every side --, a sparse and a dense
// random grid, both kinds, both metrics, the three kinds of seeds, with and without a limit.  The limited map must be the unlimited one cut at
// the limit, the tally must count every member once, and the path from the farthest voxel must end on a seed.  Prints one line per run; exits
// 0 when everything agrees.
#include "../hostcheck/geodesic_check.cpp"

#include <cstdio>

static uint32_t g_state = 2463534242u;
static uint32_t next() { return g_state = g_state * 1664525u + 1013904223u; }

int main()
{
    const uint32_t sides[] = {1u, 2u, 7u, 9u, 16u, 27u};
    for (uint32_t N : sides)
        for (uint32_t density = 3; density <= 7u; density += 4u) {
            const uint32_t n3 = N * N * N;
            std::vector<uint8_t> g(n3), mask(n3);
            for (uint8_t& v : g) v = next() % 10u < density ? (uint8_t)(1u + next() % 255u) : 0;
            for (uint8_t& v : mask) v = next() % 97u == 0u ? 0x40 : 0;
            std::vector<uint32_t> list;
            for (uint32_t k = 0; k < 5u; ++k) list.push_back(next() % n3);
            list.push_back(list[0]);                                    // a duplicate
            for (int of = 0; of < 2; ++of)
                for (int metric = 0; metric < 2; ++metric)
                    for (int kind = 0; kind < 3; ++kind) {
                        const void* seeds = kind == GEO_SEEDS_LIST ? (const void*)list.data() : kind == GEO_SEEDS_MASK ? (const void*)mask.data() : nullptr;
                        const uint32_t count = kind == GEO_SEEDS_LIST ? (uint32_t)list.size() : 0u;
                        std::vector<uint32_t> map(n3), cut(n3), path(n3);
                        uint64_t tally[5], limited[5], work[2];
                        if (gc_geodesic(g.data(), N, of, metric, kind, seeds, count, 0u, map.data(), tally, work)) { fprintf(stderr, "refused\n"); return 1; }
                        uint64_t members = 0;
                        for (uint32_t v = 0; v < n3; ++v) members += geo_member(g[v], of) ? 1u : 0u;
                        if (tally[1] + tally[2] != members) { fprintf(stderr, "N %u: the tally counts %llu of %llu members\n", N, (unsigned long long)(tally[1] + tally[2]), (unsigned long long)members); return 1; }
                        const uint32_t limit = (uint32_t)tally[3] / 2u + 1u;
                        if (gc_geodesic(g.data(), N, of, metric, kind, seeds, count, limit, cut.data(), limited, work + 0)) { fprintf(stderr, "refused\n"); return 1; }
                        for (uint32_t v = 0; v < n3; ++v)
                            if (cut[v] != (map[v] < kGeoUnreached && map[v] > limit ? kGeoUnreached : map[v])) { fprintf(stderr, "N %u: voxel %u under limit %u\n", N, v, limit); return 1; }
                        uint32_t length = 0;
                        if (tally[1]) {
                            if (gc_path(map.data(), N, metric, (uint32_t)tally[4], path.data(), n3, &length) || !length || map[path[length - 1u]] != 0u || path[0] != (uint32_t)tally[4]) {
                                fprintf(stderr, "N %u: the path from voxel %llu\n", N, (unsigned long long)tally[4]);
                                return 1;
                            }
                        } else if (tally[4] != 0xFFFFFFFFu || tally[3] != 0u) return 1;
                        printf("N %u density %u of %d metric %d seeds %d: used %llu reached %llu unreached %llu farthest %llu, path of %u\n", N, density, of, metric, kind,
                               (unsigned long long)tally[0], (unsigned long long)tally[1], (unsigned long long)tally[2], (unsigned long long)tally[3], length);
                    }
        }
    uint64_t tally[5], work[2];
    std::vector<uint8_t> g(8, 1);
    std::vector<uint32_t> map(8);
    const uint32_t outside[] = {3u, 8u};
    if (gc_geodesic(g.data(), 2, 0, 0, GEO_SEEDS_LIST, outside, 2u, 0u, map.data(), tally, work) != 1) { fprintf(stderr, "an index outside the grid accepted\n"); return 1; }
    return 0;
}
