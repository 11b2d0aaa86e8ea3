// mesh_distance.hip -- the exact distance from every voxel centre of a frame's last launch to the mesh (dxv_mesh_distance.h has the rule
// and the cull rule's margin): a nearest-triangle query over the two-box Node hierarchy, the second classic use of that tree.
//   k_mesh_distance        one thread per voxel, one wave per 4 x 4 x 4 brick, ONE walk per wave: the 64 centres of a brick are within
//                          3.5 voxels of each other and want the same subtrees, so the wave visits the union of what its lanes want
//                          (a child is entered when any lane cannot cull it).  Node index, stack and leaf index are wave-uniform:
//                          the 64-byte node and the 48-byte triangle record come through the scalar cache, one fetch per wave, the
//                          stack is one 64-entry LDS column of the wave and no lane ever diverges.  Nearest child first, by the
//                          vote of the lanes; a leaf child is tested where it is met by every lane (a minimum takes no harm from
//                          more terms); an internal far child is pushed without its bound and culled, if it can be, by its own
//                          children's bounds when it is popped.  No separate probe: the descent to the first leaf gives every lane
//                          its first upper bound, from a triangle near its brick.
//   k_mesh_distance_brute  every triangle for every voxel (option mdistwalk = 0): the on-device cross-check.
// Neither uses scratch memory; the walk's LDS is 256 bytes per workgroup.
#include "dxv_device.h"
#include "dxv_math.h"
#include "dxv_mesh_distance.h"

namespace dxv {

struct MdVoxel {
    float px, py, pz;
    size_t id;
    bool valid;
};

// the voxel of this lane: bricks x fastest, then y, then z over the launch's nz slices; a lane outside the grid (N or nz no multiple of
// 4) works on the nearest voxel inside -- it stays in the wave's votes and stores nothing
__device__ __forceinline__ MdVoxel md_voxel(const MeshDistanceParams& p)
{
    const uint32_t nb = (p.N + 3u) / 4u;
    const uint32_t bx = blockIdx.x % nb, by = (blockIdx.x / nb) % nb, bz = blockIdx.x / (nb * nb);
    const uint32_t t = threadIdx.x;
    uint32_t ix = bx * 4u + (t & 3u), iy = by * 4u + ((t >> 2) & 3u), lz = bz * 4u + (t >> 4);
    MdVoxel v;
    v.valid = ix < p.N && iy < p.N && lz < p.nz;
    ix = ix < p.N ? ix : p.N - 1u;
    iy = iy < p.N ? iy : p.N - 1u;
    lz = lz < p.nz ? lz : p.nz - 1u;
    ray_origin(p.N, ix, iy, p.z0 + lz, v.px, v.py, v.pz);
    v.id = ((size_t)lz * p.N + iy) * p.N + ix;
    return v;
}

__device__ __forceinline__ void md_store(const MeshDistanceParams& p, const MdVoxel& v, const MdBest& best)
{
    if (!v.valid) return;
    p.field[v.id] = md_value(best.d2, p.grid[v.id] != 0, p.format, p.N);
    if (p.tris) p.tris[v.id] = best.tri;
}

__global__ __launch_bounds__(64) void k_mesh_distance(const Node* __restrict__ nodes, const TriPos* __restrict__ triPos, MeshDistanceParams p)
{
    __shared__ int32_t stack[kMdStack];                                 // (the host refuses trees higher than kMdStack: one pending sibling per level)
    const MdVoxel v = md_voxel(p);
    MdBest best{p.cap, kMdNoTriangle};
    int sp = 0;
    int32_t node = 0;
    for (;;) {
        const Node& n = nodes[__builtin_amdgcn_readfirstlane(node)];
        const float lb0 = md_box_lb(v.px, v.py, v.pz, n.lo0x, n.lo0y, n.lo0z, n.hi0x, n.hi0y, n.hi0z);
        const float lb1 = md_box_lb(v.px, v.py, v.pz, n.lo1x, n.lo1y, n.lo1z, n.hi1x, n.hi1y, n.hi1z);
        const bool near0 = __popcll(__ballot(lb0 <= lb1)) >= 32;
        const int32_t cA = near0 ? n.c0 : n.c1, cB = near0 ? n.c1 : n.c0;
        const float lbA = near0 ? lb0 : lb1, lbB = near0 ? lb1 : lb0;
        int32_t next = kNoChild;
        if (__ballot(!md_cull(lbA, best.d2, kMdCullRel, p.cullAbs))) {
            if (cA < 0) md_take(best, v.px, v.py, v.pz, triPos[__builtin_amdgcn_readfirstlane(~cA)]);
            else next = cA;
        }
        if (__ballot(!md_cull(lbB, best.d2, kMdCullRel, p.cullAbs))) {  // (after the near leaf: its triangle may have culled the far child)
            if (cB < 0) md_take(best, v.px, v.py, v.pz, triPos[__builtin_amdgcn_readfirstlane(~cB)]);
            else if (next == kNoChild) next = cB;
            else if (sp < kMdStack) stack[sp++] = cB;                   // (always, for a tree no higher than its header says: never a write outside the column)
        }
        if (next == kNoChild) {
            if (!sp) break;
            next = stack[--sp];
        }
        node = next;
    }
    md_store(p, v, best);
}

__global__ __launch_bounds__(64) void k_mesh_distance_brute(const TriPos* __restrict__ triPos, uint32_t T, MeshDistanceParams p)
{
    const MdVoxel v = md_voxel(p);
    MdBest best{p.cap, kMdNoTriangle};
    for (uint32_t k = 0; k < T; ++k) md_take(best, v.px, v.py, v.pz, triPos[k]);
    md_store(p, v, best);
}

hipError_t launch_mesh_distance(const Node* nodes, const TriPos* triPos, uint32_t T, const MeshDistanceParams& p, bool walk, hipStream_t s)
{
    const uint64_t nb = (p.N + 3u) / 4u, blocks = nb * nb * ((p.nz + 3u) / 4u);
    if (!blocks || blocks > 0x7fffffffull || !T) return hipErrorInvalidValue;
    if (walk) k_mesh_distance<<<(uint32_t)blocks, 64, 0, s>>>(nodes, triPos, p);
    else k_mesh_distance_brute<<<(uint32_t)blocks, 64, 0, s>>>(triPos, T, p);
    return hipGetLastError();
}

} // namespace dxv
