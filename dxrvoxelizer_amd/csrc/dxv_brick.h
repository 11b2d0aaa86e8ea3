// dxv_brick.h -- what the kernels over 4 x 4 x 4 bricks share on the device (traverse.hip, voxelize_lists.hip, plan_bricks.hip, dxv_debug.hip):
// the launch order's brick numbering, lane -> voxel, and the brick's epilogue.
#pragma once
#include "dxv_device.h"

namespace dxv {

__device__ __forceinline__ uint32_t compact1by2(uint32_t x)
{
    x &= 0x09249249u;
    x = (x ^ (x >> 2)) & 0x030c30c3u;
    x = (x ^ (x >> 4)) & 0x0300f00fu;
    x = (x ^ (x >> 8)) & 0xff0000ffu;
    x = (x ^ (x >> 16)) & 0x000003ffu;
    return x;
}

// Brick at position `lin` of the launch order: Morton inside 2^m-brick super-blocks (m = p.mortonBits, the largest power
// of two dividing all three brick counts), super-blocks linear; offset by the launch's brick box.
__device__ __forceinline__ void brick_of_lin(const VoxelizeParams& p, uint32_t lin, uint32_t& bx, uint32_t& by, uint32_t& bz)
{
    const uint32_t m = p.mortonBits;
    const uint32_t low = lin & ((1u << (3u * m)) - 1u), high = lin >> (3u * m);
    bx = compact1by2(low); by = compact1by2(low >> 1); bz = compact1by2(low >> 2);
    if (p.superX == 1u && p.superY == 1u) bz |= high << m;      // usual case (cubic power-of-two grid): no divisions
    else {
        bx |= (high % p.superX) << m;
        by |= ((high / p.superX) % p.superY) << m;
        bz |= (high / (p.superX * p.superY)) << m;
    }
    bx += p.bx0; by += p.by0; bz += p.bz0;
}

// The lane's number in its wave, asked for where it is wanted: the brick kernels ask again rather than keep it (or threadIdx.x) in a vector
// register through a brick's body (store_brick).
__device__ __forceinline__ uint32_t lane_id()
{
    uint32_t lane;
    asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(lane));
    return lane;
}

// lane -> voxel of brick (bx, by, bz): local coordinates, lz the local slice
__device__ __forceinline__ void brick_voxel(uint32_t bx, uint32_t by, uint32_t bz, uint32_t lane, uint32_t& ix, uint32_t& iy, uint32_t& lz)
{
    ix = bx * 4u + (lane & 3u); iy = by * 4u + ((lane >> 2) & 3u); lz = bz * 4u + (lane >> 4);
}
// ... for the brick kernels: lanes that hang over the grid's end repeat its last voxels (and store nothing: store_brick)
__device__ __forceinline__ void brick_voxel_clamped(uint32_t N, uint32_t nz, uint32_t bx, uint32_t by, uint32_t bz, uint32_t lane, uint32_t& ix, uint32_t& iy, uint32_t& lz)
{
    brick_voxel(bx, by, bz, lane, ix, iy, lz);
    ix = ix < N ? ix : N - 1u; iy = iy < N ? iy : N - 1u; lz = lz < nz ? lz : nz - 1u;
}

// The epilogue of the two brick kernels (k_voxelize_queue, k_voxelize_listed): the lane's texel, and the brick's 64 result bytes as
// 16 dwords.  `lane` is asked for again BEHIND the body by the caller (lane_id): nothing of the lane's voxel is kept in vector
// registers through the scan and the triangle tests -- held across them the coordinates cost a wave per SIMD.
// p: pointer to the launch's VoxelizeParams, wherever the kernel keeps them (k_voxelize_queue: the kernel-argument segment) -- the texel
// image's address is asked for where it is used, not in front of the branch.
template <bool TEXELS, class Params>
__device__ __forceinline__ void store_brick(Params p, uint32_t N, uint32_t nz, uint32_t bx, uint32_t by, uint32_t bz, uint32_t lane, uint8_t occ, uint32_t texel)
{
    uint8_t* grid = p->grid;
    if (TEXELS || (N & 3u) != 0u) {
        uint32_t vx, vy, vz;
        brick_voxel(bx, by, bz, lane, vx, vy, vz);
        if (vx < N && vy < N && vz < nz) {
            const size_t id = ((size_t)vz * N + vy) * N + vx;
            if (TEXELS) p->texels[id] = texel;
            if ((N & 3u) != 0u) grid[id] = occ;
        }
    }
    if ((N & 3u) == 0u) {
        // rows of 4 voxels are aligned dwords: lane r < 16 stores row (y = r & 3, z = r >> 2) from the wave's ballot
        const uint64_t m = __builtin_amdgcn_ballot_w64(occ != 0);
        const uint32_t ry = by * 4u + (lane & 3u), rz = bz * 4u + ((lane >> 2) & 3u);
        if (lane < 16u && rz < nz) {
            const uint32_t nib = (uint32_t)(m >> (4u * lane)) & 15u;
            // (a plain store: four bytes that leave non-temporally reach the fabric as partial writes -- 253 MB written per launch for
            // 29 MB of results, for 0.5 % that was inside the boxes' spread)
            *reinterpret_cast<uint32_t*>(grid + ((size_t)rz * N + ry) * N + bx * 4u) = (nib * 0x00204081u) & 0x01010101u;   // bit i -> byte i
        }
    }
}

} // namespace dxv
