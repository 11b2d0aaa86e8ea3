// The product's mesh distance routine (dxrvoxelizer_amd/csrc/dxv_mesh_distance.h) compiled for the CPU: the same text the kernels of
// mesh_distance.hip run -- as a plain loop over the triangles (the brute-force kernel's order) and through md_walk over a small
// hierarchy of two-box nodes built here (median splits, exact boxes), with the cull rule's two constants as parameters.
#include "../../dxrvoxelizer_amd/csrc/dxv_mesh_distance.h"

#include <algorithm>
#include <numeric>
#include <vector>

using namespace dxv;

static TriPos record(const float* t, uint32_t index)
{
    TriPos r{};
    r.v0 = F4{t[0], t[1], t[2], 0.0f};
    r.v1 = F4{t[3], t[4], t[5], 0.0f};
    r.v2 = F4{t[6], t[7], t[8], 0.0f};
    __builtin_memcpy(&r.v0.w, &index, 4);
    return r;
}

struct Box { float lo[3], hi[3]; };

struct Tree {
    std::vector<Node> nodes;
    std::vector<TriPos> leaves;          // in leaf order
    const float* tris;
    const uint32_t* index;
    std::vector<uint32_t> order;

    Box box(uint32_t lo, uint32_t hi) const
    {
        Box b{{INFINITY, INFINITY, INFINITY}, {-INFINITY, -INFINITY, -INFINITY}};
        for (uint32_t i = lo; i < hi; ++i)
            for (int v = 0; v < 3; ++v)
                for (int a = 0; a < 3; ++a) {
                    const float x = tris[(size_t)order[i] * 9 + v * 3 + a];
                    b.lo[a] = std::min(b.lo[a], x); b.hi[a] = std::max(b.hi[a], x);
                }
        return b;
    }
    static void store(Node& n, int side, const Box& b)
    {
        if (side == 0) { n.lo0x = b.lo[0]; n.lo0y = b.lo[1]; n.lo0z = b.lo[2]; n.hi0x = b.hi[0]; n.hi0y = b.hi[1]; n.hi0z = b.hi[2]; }
        else { n.lo1x = b.lo[0]; n.lo1y = b.lo[1]; n.lo1z = b.lo[2]; n.hi1x = b.hi[0]; n.hi1y = b.hi[1]; n.hi1z = b.hi[2]; }
    }
    // the link of the subtree over order[lo, hi): ~leaf or a node index; returns its height through h
    int32_t build(uint32_t lo, uint32_t hi, uint32_t& h)
    {
        if (hi - lo == 1) {
            leaves.push_back(record(tris + (size_t)order[lo] * 9, index[order[lo]]));
            h = 0;
            return ~(int32_t)(leaves.size() - 1);
        }
        const Box b = box(lo, hi);
        int axis = 0;
        for (int a = 1; a < 3; ++a)
            if (b.hi[a] - b.lo[a] > b.hi[axis] - b.lo[axis]) axis = a;
        const uint32_t mid = lo + (hi - lo) / 2;
        auto key = [&](uint32_t t) { return tris[(size_t)t * 9 + axis] + tris[(size_t)t * 9 + 3 + axis] + tris[(size_t)t * 9 + 6 + axis]; };
        std::nth_element(order.begin() + lo, order.begin() + mid, order.begin() + hi, [&](uint32_t x, uint32_t y) { return key(x) < key(y); });
        const int32_t me = (int32_t)nodes.size();
        nodes.push_back(Node{});
        uint32_t h0 = 0, h1 = 0;
        const Box b0 = box(lo, mid), b1 = box(mid, hi);
        const int32_t c0 = build(lo, mid, h0), c1 = build(mid, hi, h1);
        Node& n = nodes[me];
        store(n, 0, b0); store(n, 1, b1);
        n.c0 = c0; n.c1 = c1; n.h0 = h0; n.h1 = h1;
        h = std::max(h0, h1) + 1;
        return me;
    }
};

extern "C" {

// d2 and tri of V points against T triangles (tris: T x 3 x 3 floats, index: the caller's indices), every triangle in turn
int mc_brute(const float* points, uint32_t V, const float* tris, const uint32_t* index, uint32_t T, float cap, float* d2, uint32_t* tri)
{
    std::vector<TriPos> rec(T);
    for (uint32_t k = 0; k < T; ++k) rec[k] = record(tris + (size_t)k * 9, index[k]);
#pragma omp parallel for
    for (long long i = 0; i < (long long)V; ++i) {
        MdBest best{cap, kMdNoTriangle};
        for (uint32_t k = 0; k < T; ++k) md_take(best, points[i * 3], points[i * 3 + 1], points[i * 3 + 2], rec[k]);
        d2[i] = best.d2; tri[i] = best.tri;
    }
    return 0;
}

// ... through md_walk over a hierarchy built here; rel, abs: the cull rule's constants (mc_margin gives the product's).  Returns the
// tree's height, or -1 when it is too high for the walk's column.
int mc_walk(const float* points, uint32_t V, const float* tris, const uint32_t* index, uint32_t T, float cap, float rel, float abs,
            float* d2, uint32_t* tri)
{
    if (!T) return -1;
    Tree t;
    t.tris = tris; t.index = index;
    t.order.resize(T);
    std::iota(t.order.begin(), t.order.end(), 0u);
    uint32_t height = 1;
    if (T == 1) {                                                       // the builder's single-triangle node: the same leaf twice, the second box far away
        t.leaves.push_back(record(tris, index[0]));
        Node n{};
        Tree::store(n, 0, t.box(0, 1));
        Tree::store(n, 1, Box{{1e30f, 1e30f, 1e30f}, {1e30f, 1e30f, 1e30f}});
        n.c0 = n.c1 = ~0;
        t.nodes.push_back(n);
    } else if (t.build(0, T, height) != 0) return -1;
    if (height > (uint32_t)kMdStack) return -1;
#pragma omp parallel for
    for (long long i = 0; i < (long long)V; ++i) {
        int32_t stack[kMdStack];
        MdBest best{cap, kMdNoTriangle};
        md_walk(best, points[i * 3], points[i * 3 + 1], points[i * 3 + 2], t.nodes.data(), t.leaves.data(), stack, rel, abs);
        d2[i] = best.d2; tri[i] = best.tri;
    }
    return (int)height;
}

// the product's cull constants for a scene whose root box is [lo, hi]
void mc_margin(const float* lo, const float* hi, float* rel, float* abs) { *rel = kMdCullRel; *abs = md_cull_abs(lo, hi); }
float mc_cap(uint32_t N, uint32_t band) { return md_cap(N, band); }
void mc_value(const float* d2, const uint8_t* solid, size_t n, int format, uint32_t N, float* out)
{
    for (size_t i = 0; i < n; ++i) out[i] = md_value(d2[i], solid[i] != 0, format, N);
}

} // extern "C"
