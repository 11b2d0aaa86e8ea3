// The product's isosurface routines (dxrvoxelizer_amd/csrc/dxv_isosurface.h) compiled for the CPU: the same text the kernels of
// isosurface.hip run, driven here in the kernels' order -- a word of 64 cells at a time: masks and counts, the exclusive scan of the
// counts, then vertices and quads at their bases.
#include "../../dxrvoxelizer_amd/csrc/dxv_isosurface.h"

#include <vector>

using namespace dxv;

namespace {

struct Lane { float s[8]; uint32_t cx, cy, cz; bool valid; };

// the 64 cells of a word: the upper four corners of a lane are its own samples, the lower four the upper four of the lane below it
void word_cells(const float* field, uint32_t N, float iso, float P, size_t word, Lane lanes[64])
{
    const uint32_t W = iso_row_words(N), C = N + 1u;
    const size_t row = word / W;
    for (uint32_t lane = 0; lane < 64u; ++lane) {
        Lane& c = lanes[lane];
        c.cx = (uint32_t)(word % W) * 64u + lane;
        c.cy = (uint32_t)(row % C);
        c.cz = (uint32_t)(row / C);
        c.valid = c.cx <= N;
        for (int e = 0; e < 4; ++e) {
            const int32_t j = (int32_t)c.cy - 1 + (e & 1), k = (int32_t)c.cz - 1 + (e >> 1);
            c.s[(e << 1) | 1] = iso_sample(field, N, (int32_t)c.cx, j, k, iso, P);
            c.s[e << 1] = lane ? lanes[lane - 1].s[(e << 1) | 1] : iso_sample(field, N, (int32_t)c.cx - 1, j, k, iso, P);
        }
    }
}

} // namespace

// pass 1 (vb == null): returns the counts in out[0] = vertices, out[1] = triangles.  pass 2: fills vb (6 floats per vertex) and ib.
extern "C" int ic_extract(const float* field, uint32_t N, float iso, float P, int object, const float* bound, uint64_t* out, float* vb, uint32_t* ib)
{
    if (!N || N > 2048) return 1;
    const size_t words = iso_words(N);
    std::vector<uint64_t> masks(words);
    std::vector<IsoCounts> bases(words);
    std::vector<Lane> lanes(64);
    for (size_t word = 0; word < words; ++word) {
        word_cells(field, N, iso, P, word, lanes.data());
        uint64_t mask = 0;
        uint32_t quads = 0;
        for (uint32_t lane = 0; lane < 64u; ++lane) {
            const Lane& c = lanes[lane];
            if (c.valid && iso_active(c.s)) mask |= 1ull << lane;
            quads += c.valid ? iso_popc(iso_owned(c.s)) : 0u;
        }
        masks[word] = mask;
        bases[word] = IsoCounts{iso_popc(mask), quads};
    }
    uint64_t vertices = 0, quads = 0;
    for (size_t word = 0; word < words; ++word) {
        const IsoCounts n = bases[word];
        bases[word] = IsoCounts{(uint32_t)vertices, (uint32_t)quads};
        vertices += n.vertices; quads += n.quads;
    }
    out[0] = vertices; out[1] = 2 * quads;
    if (!vb) return 0;
    if (vertices > kIsoMaxCount || quads > kIsoMaxCount / 6u) return 1;
    for (size_t word = 0; word < words; ++word) {
        word_cells(field, N, iso, P, word, lanes.data());
        uint64_t bits[3] = {0, 0, 0};
        for (uint32_t lane = 0; lane < 64u; ++lane)
            for (int axis = 0; axis < 3; ++axis)
                if (lanes[lane].valid && (iso_owned(lanes[lane].s) >> axis & 1u)) bits[axis] |= 1ull << lane;
        for (uint32_t lane = 0; lane < 64u; ++lane) {
            const Lane& c = lanes[lane];
            if (!(masks[word] >> lane & 1ull)) continue;
            const uint64_t lower = (1ull << lane) - 1ull;
            IsoVertex v = iso_vertex(c.s, c.cx, c.cy, c.cz);
            if (object) iso_to_object(v, N, bound);
            float* dst = vb + 6 * (size_t)(bases[word].vertices + iso_popc(masks[word] & lower));
            dst[0] = v.px; dst[1] = v.py; dst[2] = v.pz; dst[3] = v.nx; dst[4] = v.ny; dst[5] = v.nz;
            const uint32_t owned = iso_owned(c.s);
            uint32_t quad = bases[word].quads + iso_popc(bits[0] & lower) + iso_popc(bits[1] & lower) + iso_popc(bits[2] & lower);
            for (int axis = 0; axis < 3; ++axis) {
                if (!(owned >> axis & 1u)) continue;
                iso_quad(ib + 6 * (size_t)quad, masks.data(), bases.data(), N, c.cx, c.cy, c.cz, axis, iso_inside(c.s[0]), object != 0);
                ++quad;
            }
        }
    }
    return 0;
}
