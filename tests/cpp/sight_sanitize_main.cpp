// The product's line-of-sight routines (csrc/dxv_sight.h, through tests/hostcheck/sight_check.cpp) in a program of their own, for a build with
// -fsanitize=address,undefined.  Random grids with bytes other than 0 / 1 at sides 2, 62, 64, 66 and 130 -- a row of one word that is not full,
// of exactly one word, of two and of three words with a last word of two bits -- for both kinds: all 26 directions under the smallest row group
// and under one of 16 lanes must give the same map and tally, the tally must count every member once, a subset's map must be the full map
// masked, and the edit from the map must leave nothing hidden.  sc_sight lays its mask, planes and tally out by sight_carve in an allocation of
// exactly sight_scratch_bytes and writes every block at both ends.  Prints one line per run; exits 0 when everything agrees.
#include "../hostcheck/sight_check.cpp"

#include <cstdio>

static uint32_t g_state = 2463534242u;
static uint32_t next() { return g_state = g_state * 1664525u + 1013904223u; }

int main()
{
    const uint32_t sides[] = {2u, 62u, 64u, 66u, 130u};
    for (uint32_t N : sides) {
        const size_t n3 = (size_t)N * N * N;
        std::vector<uint8_t> g(n3);
        for (uint8_t& v : g) v = (next() >> 8) % 10u < 3u ? (uint8_t)(1u + (next() >> 8) % 255u) : 0;
        for (int of = 0; of < 2; ++of) {
            std::vector<uint32_t> full(n3), wide(n3), part(n3);
            uint64_t tally[kSightTallyWords], again[kSightTallyWords];
            if (sc_sight(g.data(), N, of, kSightAll, 0u, full.data(), tally) || sc_sight(g.data(), N, of, kSightAll, 16u, wide.data(), again)) { fprintf(stderr, "refused\n"); return 1; }
            uint64_t members = 0, counted = 0;
            for (size_t v = 0; v < n3; ++v) {
                members += (of == THICK_EMPTY ? !solid(g[v]) : solid(g[v])) ? 1u : 0u;
                if (full[v] != wide[v] || (full[v] & ~kSightAll)) { fprintf(stderr, "N %u of %d: voxel %zu\n", N, of, v); return 1; }
            }
            for (uint32_t k = 0; k < kSightBits; ++k) counted += tally[41u + k];
            if (memcmp(tally, again, sizeof(tally)) || tally[0] != members || counted != members) { fprintf(stderr, "N %u of %d: the tally counts %llu of %llu members\n", N, of, (unsigned long long)counted, (unsigned long long)members); return 1; }
            printf("N %u of %d all: members %llu hidden %llu\n", N, of, (unsigned long long)members, (unsigned long long)tally[41]);
            const uint32_t some = 1u << sight_bit(-1, 1, 1) | 1u << sight_bit(1, -1, -1) | 1u << sight_bit(-1, 0, 0) | 1u << sight_bit(0, 1, 0) | 1u << sight_bit(1, 0, -1);
            if (sc_sight(g.data(), N, of, some, 0u, part.data(), again)) { fprintf(stderr, "refused\n"); return 1; }
            for (size_t v = 0; v < n3; ++v)
                if (part[v] != (full[v] & some)) { fprintf(stderr, "N %u of %d: voxel %zu of the subset\n", N, of, v); return 1; }
            std::vector<uint8_t> edited(g);
            if (sc_sight_fill(edited.data(), N, of, some, part.data()) || sc_sight(edited.data(), N, of, some, 0u, part.data(), again)) { fprintf(stderr, "refused\n"); return 1; }
            if (again[41]) { fprintf(stderr, "N %u of %d: %llu members hidden after the edit\n", N, of, (unsigned long long)again[41]); return 1; }
            printf("N %u of %d subset: members after the edit %llu\n", N, of, (unsigned long long)again[0]);
        }
    }
    uint64_t tally[kSightTallyWords];
    std::vector<uint8_t> g(8, 1);
    std::vector<uint32_t> map(8);
    if (sc_sight(g.data(), 2, 0, 0u, 0u, map.data(), tally) != 1 || sc_sight(g.data(), 2, 0, 1u << 13, 0u, map.data(), tally) != 1 || sc_sight(g.data(), 2, 2, 1u, 0u, map.data(), tally) != 1) {
        fprintf(stderr, "a bad call accepted\n");
        return 1;
    }
    return 0;
}
