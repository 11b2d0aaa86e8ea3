// The surface pass's candidate enumeration (dxrvoxelizer_amd/csrc/dxv_surface.h) compiled for the CPU: the same text the two kernels of
// surface.hip run, driven here the way they drive it -- per triangle the box clipped to the partition, then either every voxel of a small
// box or the column walk of a large one, every candidate decided by surface_overlap at the ray rule's voxel centre.
#include "../../dxrvoxelizer_amd/csrc/dxv_surface.h"

#include <cstddef>

using namespace dxv;

enum { SC_NO_BOX = 0, SC_SMALL = 1, SC_LARGE = 2 };

namespace {

struct Tally { uint32_t candidates, accepted; };

void test_voxel(const SurfaceGrid& g, const SurfaceTri& t, int ix, int iy, int iz, uint32_t lz, Tally& n)
{
    float cx, cy, cz;
    ray_origin(g.N, (uint32_t)ix, (uint32_t)iy, (uint32_t)iz, cx, cy, cz);
    ++n.candidates;
    if (surface_overlap(t.a, t.b, t.d, cx, cy, cz, g.h)) {
        g.grid[((size_t)lz * g.N + (uint32_t)iy) * g.N + (uint32_t)ix] = 1;
        ++n.accepted;
    }
}

} // namespace

// tris: 9 floats per triangle, normalised.  The partition as the library's launch states it: nz local slices from global slice z0, in
// blocks of zBlock every zPeriod (a slab: zBlock = zPeriod = nz).  grid: nz * N * N bytes, which the caller has cleared.
// forceLarge: every triangle with a box takes the column walk.  oldWalk: the walk without the far-vertex limit (what it loses is the
// point of tests/test_surface_walk.py; the kernels have no such switch).  info: per triangle the path, the candidates tested, the
// candidates accepted.  Returns non-zero for a partition that does not fit the grid.
extern "C" int sc_surface(const float* tris, uint32_t T, uint32_t N, uint32_t z0, uint32_t nz, uint32_t zBlock, uint32_t zPeriod, int forceLarge, int oldWalk,
                          uint8_t* grid, uint32_t* info)
{
    if (!N || N > 2048u || !nz || !zBlock || zPeriod < zBlock) return 1;
    SurfaceGrid g{};
    g.grid = grid; g.N = N; g.z0 = z0; g.nz = nz; g.zBlock = zBlock; g.zPeriod = zPeriod;
    const uint64_t zLast = (uint64_t)z0 + (uint64_t)((nz - 1u) / zBlock) * zPeriod + (nz - 1u) % zBlock;
    if (zLast >= N) return 1;
    g.zLast = (uint32_t)zLast;
    g.h = 1.0f / (float)N;
    for (uint32_t i = 0; i < T; ++i) {
        SurfaceTri t;
        for (int k = 0; k < 3; ++k) { t.a[k] = tris[9u * i + k]; t.b[k] = tris[9u * i + 3 + k]; t.d[k] = tris[9u * i + 6 + k]; }
        uint32_t* out = info + 3u * i;
        out[0] = SC_NO_BOX; out[1] = out[2] = 0u;
        Tally n{0u, 0u};
        int lo[3], hi[3];
        if (!tri_box(g, t, lo, hi)) continue;
        if (!forceLarge && box_is_small(lo, hi)) {
            out[0] = SC_SMALL;
            for (int z = lo[2]; z <= hi[2]; ++z)
                for (int y = lo[1]; y <= hi[1]; ++y)
                    for (int x = lo[0]; x <= hi[0]; ++x) {
                        uint32_t lz;
                        if (local_slice(g, z, lz)) test_voxel(g, t, x, y, z, lz, n);
                    }
        } else {
            out[0] = SC_LARGE;
            SurfaceCols s;
            cols_setup(g, t, lo, hi, s, !oldWalk);
            for (uint32_t col = 0; col < s.cols; ++col) {
                int iu, iv, k0, k1;
                if (!column_range(s, col, iu, iv, k0, k1)) continue;
                for (int k = k0; k <= k1; ++k) {
                    int x, y, z;
                    column_voxel(s, iu, iv, k, x, y, z);
                    uint32_t lz;
                    if (local_slice(g, z, lz)) test_voxel(g, t, x, y, z, lz, n);
                }
            }
        }
        out[1] = n.candidates; out[2] = n.accepted;
    }
    return 0;
}
