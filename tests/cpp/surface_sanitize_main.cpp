// The surface pass's candidate enumeration (csrc/dxv_surface.h, through tests/hostcheck/surface_check.cpp) in a program of its own, for a
// build with -fsanitize=address,undefined.  The triangles: the case families of tests/surface_cases.py, which the test writes into the file
// named on the command line -- per record the grid side, the number of triangles, nine floats per triangle.  Every record runs as the
// kernels choose the path, with every triangle forced down the column walk, and with the walk without the far-vertex limit; then through
// slabs and block-cyclic shares, each of which must equal its slices of the whole grid.  Prints one line per record; exits 0 when
// everything agrees.
#include "../hostcheck/surface_check.cpp"

#include <cstdio>
#include <cstring>
#include <vector>

static int run(uint32_t N, const std::vector<float>& tris)
{
    const uint32_t T = (uint32_t)(tris.size() / 9u);
    const size_t slice = (size_t)N * N;
    std::vector<uint8_t> whole(slice * N), forced(slice * N), old(slice * N);
    std::vector<uint32_t> info(3u * T + 3u), infoForced(3u * T + 3u), infoOld(3u * T + 3u);
    if (sc_surface(tris.data(), T, N, 0u, N, N, N, 0, 0, whole.data(), info.data())) return 1;
    if (sc_surface(tris.data(), T, N, 0u, N, N, N, 1, 0, forced.data(), infoForced.data())) return 1;
    if (sc_surface(tris.data(), T, N, 0u, N, N, N, 1, 1, old.data(), infoOld.data())) return 1;
    if (whole != forced) { fprintf(stderr, "N %u: the forced walk differs\n", N); return 1; }
    uint64_t set = 0, lost = 0, candidates = 0;
    for (size_t v = 0; v < whole.size(); ++v) {
        set += whole[v];
        lost += whole[v] && !old[v];
        if (old[v] && !whole[v]) { fprintf(stderr, "N %u: the walk without the limit sets voxel %zu\n", N, v); return 1; }
    }
    for (uint32_t i = 0; i < T; ++i) candidates += info[3u * i + 1u];
    uint32_t parts = 0;
    const uint32_t slabs[3][2] = {{13u, 9u}, {0u, 1u}, {N - 5u, 5u}};
    for (const auto& s : slabs) {
        if (s[0] + s[1] > N) continue;
        std::vector<uint8_t> g(slice * s[1]);
        if (sc_surface(tris.data(), T, N, s[0], s[1], s[1], s[1], 0, 0, g.data(), infoOld.data())) return 1;
        if (memcmp(g.data(), whole.data() + slice * s[0], g.size())) { fprintf(stderr, "N %u: slab %u+%u\n", N, s[0], s[1]); return 1; }
        ++parts;
    }
    for (uint32_t world = 2; world <= 8u; world += 6u)
        for (uint32_t zBlock = 4; zBlock <= 8u; zBlock += 4u)
            for (uint32_t rank = 0; rank < world; ++rank) {
                std::vector<uint32_t> zs;
                for (uint32_t z = 0; z < N; ++z)
                    if ((z / zBlock) % world == rank) zs.push_back(z);
                if (zs.empty()) continue;
                std::vector<uint8_t> g(slice * zs.size());
                if (sc_surface(tris.data(), T, N, rank * zBlock, (uint32_t)zs.size(), zBlock, zBlock * world, 0, 0, g.data(), infoOld.data())) return 1;
                for (size_t lz = 0; lz < zs.size(); ++lz)
                    if (memcmp(g.data() + slice * lz, whole.data() + slice * zs[lz], slice)) { fprintf(stderr, "N %u: share %u/%u of blocks of %u, slice %u\n", N, rank, world, zBlock, zs[lz]); return 1; }
                ++parts;
            }
    printf("N %u triangles %u: %llu voxels from %llu candidates, %llu lost without the limit, %u partitions\n", N, T, (unsigned long long)set, (unsigned long long)candidates,
           (unsigned long long)lost, parts);
    return 0;
}

int main(int argc, char** argv)
{
    if (argc != 2) { fprintf(stderr, "usage: %s cases.bin\n", argv[0]); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
    uint32_t head[2], records = 0;
    while (fread(head, sizeof(uint32_t), 2, f) == 2) {
        if (head[0] < 6u || head[0] > 128u || head[1] > 4096u) { fprintf(stderr, "a record of side %u with %u triangles\n", head[0], head[1]); return 2; }
        std::vector<float> tris(9u * (size_t)head[1]);
        if (fread(tris.data(), sizeof(float), tris.size(), f) != tris.size()) { fprintf(stderr, "a short record\n"); return 2; }
        if (run(head[0], tris)) return 1;
        ++records;
    }
    fclose(f);
    if (!records) { fprintf(stderr, "no record in %s\n", argv[1]); return 2; }
    // a partition that does not fit the grid is refused
    std::vector<uint8_t> g(64);
    uint32_t info[3];
    const float one[9] = {0, 0, 0, 0.5f, 0, 0, 0, 0.5f, 0};
    if (sc_surface(one, 1u, 4u, 2u, 3u, 3u, 3u, 0, 0, g.data(), info) != 1 || sc_surface(one, 1u, 4u, 0u, 2u, 2u, 1u, 0, 0, g.data(), info) != 1) {
        fprintf(stderr, "a partition outside the grid accepted\n");
        return 1;
    }
    return 0;
}
