// The product's thickness routines (csrc/dxv_thickness.h, through tests/hostcheck/thickness_check.cpp) in a program of their own, for a build
// with -fsanitize=address,undefined: sides 2, 6 and 66, a seeded union of balls and a sparse random grid, both kinds, every value of thickcull.
// The four culls must give the same map and histogram, and the histogram must count every voxel once.  Prints one line per run; exits 0 when
// everything agrees.
#include "../hostcheck/thickness_check.cpp"

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
        for (uint8_t& v : g) v = next() % 10u == 0u ? 1 : 0;
    }
    return g;
}

int main()
{
    const uint32_t sides[] = {2u, 6u, 66u}, caps[] = {2u, 6u, 101u, 4096u};
    for (uint32_t N : sides)
        for (int what = 0; what < 2; ++what) {
            const std::vector<uint8_t> g = make_grid(N, what);
            const size_t n3 = g.size();
            for (uint32_t cap : caps) {
                if (cap > 101u && N > 6u) continue;                     // (the largest balls only where the grid is small: the program is meant to be quick)
                for (int of = 0; of < 2; ++of) {
                    std::vector<uint32_t> first(n3), W(n3);
                    std::vector<uint64_t> firstHist(cap + 1u), hist(cap + 1u);
                    uint64_t counters[2] = {0, 0};
                    for (uint32_t cull = 0; cull < 4u; ++cull) {
                        if (tc_thickness(g.data(), N, of, cap, cull, W.data(), hist.data(), counters)) { fprintf(stderr, "refused\n"); return 1; }
                        uint64_t sum = 0;
                        for (uint64_t h : hist) sum += h;
                        if (sum != n3) { fprintf(stderr, "N %u: the histogram counts %llu of %zu voxels\n", N, (unsigned long long)sum, n3); return 1; }
                        if (cull == 0u) { first = W; firstHist = hist; }
                        else if (W != first || hist != firstHist) { fprintf(stderr, "N %u cap %u of %d: thickcull %u differs from 0\n", N, cap, of, cull); return 1; }
                    }
                    printf("N %u grid %d cap %u of %d: members %llu, painted with both culls %llu centres %llu items\n", N, what, cap, of,
                           (unsigned long long)(n3 - hist[0]), (unsigned long long)counters[0], (unsigned long long)counters[1]);
                }
            }
        }
    return 0;
}
