// sight.hip -- the line-of-sight map of a whole N^3 grid (dxv_sight.h has the rule and the word routines), on the frame's stream.  A fixed
// chain of kernels, nothing for the host to settle:
//   k_sight_pack     grid (1 B per voxel) -> the member mask M (1 bit per voxel, the fill's layout; the complement inside the grid for the
//                    empty kind): the one read of the grid, eight bytes per thread
//   k_sight_sweep    ONE launch for all requested directions, the direction in blockIdx.y: M -> the plane V_d.  Along z or y a lane owns one
//                    word of one line family; the lanes of a row sit side by side in a group of 1, 2, 4, 8 or 16, and where dx != 0 a word's
//                    carry comes from the lane beside it by a shuffle inside the group.  A family's addresses do not depend on the values:
//                    the loads of kSightBlock steps are issued together and the chain runs through registers.  Along x alone a lane scans one
//                    row.  Every word of every plane is stored exactly once, aligned: nothing is cleared, nothing is atomic
//   k_sight_map      the planes -> the map: a wave per eight mask words, lane p loads plane p's words (one vector load per mask word, eight in
//                    flight), each word is handed round the wave, lane x builds voxel x's uint32; the store is a whole-wave access
//   k_sight_tally    M and the planes -> the 68 integers, a thread per mask word in a grid-stride loop: popcounts and the bit-sliced counter
//                    of dxv_sight.h in 32-bit shares, reduced in the wave, then through LDS, then one set of 64-bit atomics per workgroup
//   k_sight_fill     the edit: map and grid -> the grid in place, a thread per voxel, a store only where a voxel changes kind
// No workgroup waits for another, every loop is bounded by N; launch sizes depend on N and the directions alone.  The tally's words, M and the
// planes are laid out by sight_carve (dxv_sight.h).
#include "dxv_device.h"
#include "dxv_sight.h"

namespace dxv {

constexpr uint32_t kSightMapBlocks = 8192;        // workgroups (of four waves) the map is launched with at the most
constexpr uint32_t kSightMapWords = 8;            // mask words a wave takes per trip: their planes' loads are in flight together
constexpr uint32_t kSightTallyBlocks = 1024;      // ... the tally

// one thread per byte of a mask row (W * 8 of them, the ones behind the row's end are 0)
__global__ __launch_bounds__(256) void k_sight_pack(const uint8_t* __restrict__ grid, uint32_t N, int of, uint8_t* __restrict__ mask)
{
    const uint32_t rowBytes = fill_row_words(N) * 8u;
    const size_t t = (size_t)blockIdx.x * 256u + threadIdx.x;
    if (t >= (size_t)N * N * rowBytes) return;
    const size_t row = t / rowBytes;
    const uint32_t j = (uint32_t)(t % rowBytes);
    uint32_t bits = 0;
    if (8u * j < N) {
        const uint8_t* g = grid + row * N;
        bits = (N & 7u) ? sight_member_byte(g, N, j, of) : sight_member_byte(*reinterpret_cast<const uint64_t*>(g + 8u * j), of);
    }
    mask[t] = (uint8_t)bits;
}

// blockIdx.y: the plane, i.e. the requested direction of that rank.  G: the lanes of a row group (a power of two, W <= G <= 16; 256 % G == 0, so
// a group never straddles a wave and every lane of a group leaves or stays together).
__global__ __launch_bounds__(256) void k_sight_sweep(const uint64_t* __restrict__ mask, uint32_t N, uint32_t directions, uint32_t G, uint64_t* __restrict__ planes)
{
    uint32_t rest = directions;
    for (uint32_t p = 0; p < blockIdx.y; ++p) rest &= rest - 1u;
    const uint32_t b = sight_lowest(rest), W = fill_row_words(N);
    const SightSweep s = sight_sweep(b, N);
    uint64_t* __restrict__ plane = planes + (size_t)blockIdx.y * fill_mask_words(N);
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    if (s.axis == 0) {                                                  // along x alone: a lane per row
        if (t >= s.families) return;
        sight_row_x(mask + (size_t)t * W, plane + (size_t)t * W, N, W, s.dx);
        return;
    }
    const uint32_t f = t / G, w = t % G;
    if (f >= s.families) return;
    const bool mine = w < W;                                            // (the group's spare lanes stay for the shuffles)
    uint64_t V = ~0ull;
    for (uint32_t done = 0; done < N; done += kSightBlock) {
        uint64_t m[kSightBlock];
#pragma unroll
        for (uint32_t j = 0; j < kSightBlock; ++j) {
            const uint32_t k = done + j;
            const int32_t row = sight_row_at(s, N, f, k);
            m[j] = mine && k < N && (uint32_t)row < N ? mask[(size_t)sight_step_at(s, N, k) * s.stepStride + (size_t)row * s.rowStride + w] : 0ull;
        }
#pragma unroll
        for (uint32_t j = 0; j < kSightBlock; ++j) {
            const uint32_t k = done + j;
            if (k >= N) break;                                          // (the same for every lane)
            uint32_t in = sight_carry(V, s.dx);
            if (s.dx > 0) in = (uint32_t)__shfl_up((int)in, 1u, (int)G);
            else if (s.dx < 0) in = (uint32_t)__shfl_down((int)in, 1u, (int)G);
            const int32_t row = sight_row_at(s, N, f, k);
            if ((uint32_t)row >= N) { V = ~0ull; continue; }            // outside the grid: all ones
            V = sight_step(m[j], V, in, s.dx, N, w, W);
            if (mine) plane[(size_t)sight_step_at(s, N, k) * s.stepStride + (size_t)row * s.rowStride + w] = V;
        }
    }
}

// word `lane` of the wave, handed to every lane
__device__ __forceinline__ uint64_t sight_hand_round(uint64_t v, uint32_t lane)
{
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, (int)lane), hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), (int)lane);
    return (uint64_t)hi << 32 | lo;
}

__global__ __launch_bounds__(256) void k_sight_map(const uint64_t* __restrict__ planes, uint32_t N, uint32_t directions, uint32_t* __restrict__ map)
{
    const uint32_t W = fill_row_words(N), words = N * N * W, lane = threadIdx.x & 63u, count = sight_popc(directions);
    const uint32_t trips = (words + kSightMapWords - 1u) / kSightMapWords;
    for (uint32_t trip = blockIdx.x * 4u + (threadIdx.x >> 6); trip < trips; trip += gridDim.x * 4u) {
        const uint32_t first = trip * kSightMapWords;
        uint64_t mine[kSightMapWords];
#pragma unroll
        for (uint32_t j = 0; j < kSightMapWords; ++j) mine[j] = lane < count && first + j < words ? planes[(size_t)lane * words + first + j] : 0ull;
#pragma unroll
        for (uint32_t j = 0; j < kSightMapWords; ++j) {
            const uint32_t u = first + j;
            if (u >= words) break;                                      // (the same for every lane)
            uint32_t word = 0, p = 0;
            for (uint32_t left = directions; left; left &= left - 1u, ++p)
                word |= sight_map_bit(sight_hand_round(mine[j], p), lane, sight_lowest(left));
            const uint32_t row = u / W, x = (u - row * W) * 64u + lane;
            if (x < N) map[(size_t)row * N + x] = word;
        }
    }
}

__global__ __launch_bounds__(256) void k_sight_tally(const uint64_t* __restrict__ mask, const uint64_t* __restrict__ planes, uint32_t words, uint32_t directions,
                                                     unsigned long long* __restrict__ tally)
{
    __shared__ uint32_t part[4][kSightTallyWords];
    SightTallyOf<uint32_t> t{};                                         // (a thread's share: at most 64 a word, a few hundred words)
    for (uint32_t u = blockIdx.x * 256u + threadIdx.x; u < words; u += gridDim.x * 256u) {
        uint64_t v[kSightBits];
        uint32_t p = 0;
#pragma unroll
        for (uint32_t b = 0; b < kSightBits; ++b) {
            const bool asked = directions >> b & 1u;
            v[b] = asked ? planes[(size_t)p * words + u] : 0ull;
            p += asked ? 1u : 0u;
        }
        sight_tally_word(t, mask[u], v, directions);
    }
    uint32_t* share = reinterpret_cast<uint32_t*>(&t);
#pragma unroll
    for (uint32_t k = 0; k < kSightTallyWords; ++k) {
        uint32_t sum = share[k];
#pragma unroll
        for (uint32_t d = 1; d < 64u; d <<= 1) sum += (uint32_t)__shfl_xor((int)sum, (int)d);
        if ((threadIdx.x & 63u) == 0u) part[threadIdx.x >> 6][k] = sum;
    }
    __syncthreads();
    if (threadIdx.x >= kSightTallyWords) return;
    const unsigned long long sum = (unsigned long long)part[0][threadIdx.x] + part[1][threadIdx.x] + part[2][threadIdx.x] + part[3][threadIdx.x];
    if (sum) (void)__hip_atomic_fetch_add(tally + threadIdx.x, sum, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ __launch_bounds__(256) void k_sight_fill(uint8_t* grid, const uint32_t* __restrict__ map, uint32_t voxels, int of, uint32_t directions)
{
    const uint32_t v = blockIdx.x * 256u + threadIdx.x;
    if (v < voxels && sight_fill_changes(grid[v], map[v], of, directions)) grid[v] = sight_fill_byte(of);
}

// l: sight_carve(N, directions) over the call's scratch.  group: option sightgroup
hipError_t launch_sight(const uint8_t* grid, uint32_t N, int of, uint32_t directions, uint32_t group, uint32_t* map, const SightScratch& l, hipStream_t s)
{
    if (!grid || !map || !l.tally || !l.mask || !l.planes || !sight_valid(N, of, directions) || group > kSightMaxGroup || (group & (group - 1u))) return hipErrorInvalidValue;
    const hipError_t e = hipMemsetAsync(l.tally, 0, kSightTallyWords * sizeof(unsigned long long), s);
    if (e != hipSuccess) return e;
    const uint32_t W = fill_row_words(N), words = N * N * W, G = sight_group(W, group);     // (N <= kSightMaxN: 2^24 words at the most)
    k_sight_pack<<<(uint32_t)(((size_t)words * 8u + 255u) / 256u), 256, 0, s>>>(grid, N, of, reinterpret_cast<uint8_t*>(l.mask));
    uint32_t lanes = 0;
    for (uint32_t left = directions; left; left &= left - 1u) {
        const SightSweep sw = sight_sweep(sight_lowest(left), N);
        const uint32_t need = sw.axis ? sw.families * G : sw.families;
        if (need > lanes) lanes = need;
    }
    k_sight_sweep<<<dim3((lanes + 255u) / 256u, sight_popc(directions)), 256, 0, s>>>(l.mask, N, directions, G, l.planes);
    const uint32_t trips = (words + kSightMapWords - 1u) / kSightMapWords, mapBlocks = (trips + 3u) / 4u, tallyBlocks = (words + 255u) / 256u;
    k_sight_map<<<mapBlocks < kSightMapBlocks ? mapBlocks : kSightMapBlocks, 256, 0, s>>>(l.planes, N, directions, map);
    k_sight_tally<<<tallyBlocks < kSightTallyBlocks ? tallyBlocks : kSightTallyBlocks, 256, 0, s>>>(l.mask, l.planes, words, directions, l.tally);
    return hipGetLastError();
}

hipError_t launch_sight_fill(uint8_t* grid, uint32_t N, int of, uint32_t directions, const uint32_t* map, hipStream_t s)
{
    if (!grid || !map || !sight_valid(N, of, directions)) return hipErrorInvalidValue;
    const uint32_t voxels = N * N * N;
    k_sight_fill<<<(voxels + 255u) / 256u, 256, 0, s>>>(grid, map, voxels, of, directions);
    return hipGetLastError();
}

} // namespace dxv
