// geodesic.hip -- the geodesic distance inside a whole N^3 grid (dxv_geodesic.h has the rule and the routines), on the frame's stream:
//   k_geo_init      grid (1 B per voxel) and the seeds -> the map's first words (0 on a seed that is a member, kGeoUnreached on the other members,
//                   kGeoNone elsewhere) and the live flags of round 0: every tile that holds a seed or a neighbour of one
//   k_geo_seed_list ... the seeds of a list, behind an init without seeds
//   k_geo_compact   a round's live flags -> its queue of tiles and their number (word `round` of the control block); clears the flags it read
//   k_geo_round     a wave per queued tile, tiles dealt in a bounded grid-stride loop: the tile and its halo from the map into LDS (10^3 words),
//                   relaxed there until a wave-wide vote says nothing changed, the words that changed back into the map, and in the NEXT round's
//                   flags every neighbour tile that borders one of them
//   k_geo_tally     the map -> seeds used, reached, unreached, the farthest voxel
//   k_geo_path      one wave: from a target down to a seed
// A batch is `rounds` rounds behind one another.  The kernels of a round return at once when the round before left nothing live, so a batch
// costs what its live rounds cost, and the host reads the block where the frame is next synchronised (dxv_products.hip: settle_geodesic).
// A tile reads its neighbours' words while they may be lowering them: every word ever stored is the length of a real path and words only fall,
// so a stale word is a valid upper bound, and whoever lowers a word on a tile's border flags the tiles beyond it for the next round -- the
// chain stops only at the fixed point, which is unique.  No workgroup waits for another, every loop is bounded, launch sizes
// depend on N alone; no scratch memory.  Control block, flags and queue are laid out by geodesic_carve (dxv_geodesic.h).
#include "dxv_device.h"
#include "dxv_geodesic.h"

namespace dxv {

constexpr uint32_t kGeoRoundBlocks = 8192;        // workgroups (of one wave) a round is launched with at the most, whatever its queue holds
constexpr uint32_t kGeoTallyBlocks = 1024;        // ... the tally, of four waves

// one thread per voxel
__global__ __launch_bounds__(256) void k_geo_init(const uint8_t* __restrict__ grid, uint32_t N, int of, int seedsKind, const uint8_t* __restrict__ seedMask, uint32_t* __restrict__ map,
                                                  uint8_t* __restrict__ live)
{
    const size_t v = (size_t)blockIdx.x * 256u + threadIdx.x;
    if (v >= (size_t)N * N * N) return;
    const uint32_t row = (uint32_t)(v / N), x = (uint32_t)(v - (size_t)row * N), y = row % N, z = row / N;
    const bool seed = seedsKind == GEO_SEEDS_BORDER ? geo_border(x, y, z, N) : seedsKind == GEO_SEEDS_MASK ? seedMask[v] != 0 : false;
    const uint32_t word = geo_start(grid[v], of, seed);
    map[v] = word;
    if (!word) geo_mark_seed(live, geo_tiles_side(N), x, y, z);         // (the same byte from every seed of a tile)
}

// one thread per entry of the list; duplicates store the same words
__global__ __launch_bounds__(256) void k_geo_seed_list(const uint32_t* __restrict__ seeds, uint32_t count, uint32_t N, uint32_t* __restrict__ map, uint8_t* __restrict__ live)
{
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    if (t >= count) return;
    const uint32_t v = seeds[t];
    if (v >= N * N * N || map[v] == kGeoNone) return;                   // (the host has refused an index outside the grid; a seed that is no member is ignored)
    const uint32_t row = v / N;
    map[v] = 0u;
    geo_mark_seed(live, geo_tiles_side(N), v - row * N, row % N, row / N);
}

// one thread per tile: the queue's order is whatever the atomics make it, and does not matter
__global__ __launch_bounds__(256) void k_geo_compact(uint8_t* __restrict__ live, uint32_t tiles, GeoControl* __restrict__ ctl, uint32_t round, uint32_t* __restrict__ queue)
{
    if (round && ctl->live[round - 1u] == 0u) return;
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    const bool mine = t < tiles && live[t] != 0;
    if (mine) live[t] = 0;                                              // (the round after the next one marks into these flags)
    const unsigned long long votes = __ballot(mine);
    if (!votes) return;
    const uint32_t lane = threadIdx.x & 63u, leader = (uint32_t)__ffsll(votes) - 1u;
    uint32_t base = 0;
    if (lane == leader) base = atomicAdd(&ctl->live[round], (uint32_t)__popcll(votes));
    base = (uint32_t)__shfl((int)base, (int)leader);
    const uint32_t at = base + (uint32_t)__popcll(votes & ((1ull << lane) - 1ull));
    if (mine && at < tiles) queue[at] = t;                              // (at < tiles: a tile is queued once)
}

// One wave per tile.  Lane (ly, lx) owns the column of eight voxels along z: a b32 access of the wave then touches banks 10 ly + lx + const, which
// are distinct within each half of the wave (0 .. 37 and 40 .. 77 mod 64).
template <int kMetric> __global__ __launch_bounds__(64) void k_geo_round(uint32_t* map, uint32_t N, uint32_t limit, const GeoControl* __restrict__ ctl, uint32_t round,
                                                                         const uint32_t* __restrict__ queue, uint8_t* __restrict__ next)
{
    __shared__ uint32_t T[kGeoTileWords];
    __shared__ uint32_t touched;
    const uint32_t side = geo_tiles_side(N), tiles = side * side * side;
    uint32_t count = ctl->live[round];
    if (count > tiles) count = tiles;
    const uint32_t lane = threadIdx.x, lx = lane & 7u, ly = lane >> 3;
    for (uint32_t i = blockIdx.x; i < count; i += gridDim.x) {
        const uint32_t tile = queue[i];
        if (tile >= tiles) continue;                                    // (never: what k_geo_compact wrote is a tile of the grid)
        const uint32_t tx = tile % side, ty = tile / side % side, tz = tile / (side * side);
        if (lane == 0u) touched = 0u;
        for (uint32_t w = lane; w < kGeoTileWords; w += 64u) {
            const uint32_t v = geo_tile_voxel(tx, ty, tz, w, N);
            T[w] = v != kGeoNone ? map[v] : kGeoNone;
        }
        __syncthreads();
        uint32_t orig[kGeoTile];
#pragma unroll
        for (uint32_t z = 0; z < kGeoTile; ++z) orig[z] = T[geo_tile_at(lx, ly, z)];
        bool unsettled = true;
        for (uint32_t sweep = 0; sweep < kGeoMaxSweeps; ++sweep) {
            bool changed = false;
#pragma unroll
            for (uint32_t z = 0; z < kGeoTile; ++z) {
                const uint32_t at = geo_tile_at(lx, ly, z), cur = T[at], v = geo_relax<kMetric>(T, at, cur, limit);
                if (v != cur) { T[at] = v; changed = true; }
            }
            __syncthreads();
            if (!__any(changed)) { unsettled = false; break; }
        }
        uint32_t mask = unsettled ? 1u << kGeoSelf : 0u;                // (never: the sweeps' bound is the relaxation's own; then the tile runs again)
#pragma unroll
        for (uint32_t z = 0; z < kGeoTile; ++z) {
            const uint32_t v = T[geo_tile_at(lx, ly, z)];
            if (v == orig[z]) continue;
            map[geo_tile_voxel(tx, ty, tz, geo_tile_at(lx, ly, z), N)] = v;     // (a word that changed is a member's: inside the grid)
            mask |= geo_touch(lx, ly, z, kMetric);
        }
        if (mask) atomicOr(&touched, mask);
        __syncthreads();
        if (lane < 27u && (touched >> lane & 1u)) {
            const uint32_t nx = tx + (uint32_t)geo_slot_dx(lane), ny = ty + (uint32_t)geo_slot_dy(lane), nz = tz + (uint32_t)geo_slot_dz(lane);
            if (nx < side && ny < side && nz < side) next[(nz * side + ny) * side + nx] = 1;
        }
        __syncthreads();                                                // (the next tile's load overwrites T and `touched`)
    }
}

__global__ __launch_bounds__(256) void k_geo_tally(const uint32_t* __restrict__ map, uint32_t voxels, GeoControl* __restrict__ ctl)
{
    __shared__ GeoTally part[4];
    GeoTally t{0, 0, 0, 0};
    for (uint32_t v = blockIdx.x * 256u + threadIdx.x; v < voxels; v += gridDim.x * 256u) geo_tally_voxel(t, map[v], v);
#pragma unroll
    for (uint32_t d = 1; d < 64u; d <<= 1) {
        const GeoTally o{__shfl_xor(t.seeds, d), __shfl_xor(t.reached, d), __shfl_xor(t.unreached, d), __shfl_xor(t.key, d)};
        geo_tally_combine(t, o);
    }
    if ((threadIdx.x & 63u) == 0u) part[threadIdx.x >> 6] = t;
    __syncthreads();
    if (threadIdx.x) return;
    for (uint32_t k = 1; k < 4u; ++k) geo_tally_combine(t, part[k]);
    if (t.seeds) (void)__hip_atomic_fetch_add(&ctl->tally[0], t.seeds, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (t.reached) (void)__hip_atomic_fetch_add(&ctl->tally[1], t.reached, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (t.unreached) (void)__hip_atomic_fetch_add(&ctl->tally[2], t.unreached, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (t.key) (void)__hip_atomic_fetch_max(&ctl->tally[3], t.key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// One wave.  Every step lowers the word by at least 1, so the word of the target bounds the steps.
__global__ __launch_bounds__(64) void k_geo_path(const uint32_t* __restrict__ map, uint32_t N, int metric, uint32_t target, uint32_t* __restrict__ out, uint32_t capacity)
{
    const uint32_t lane = threadIdx.x;
    uint32_t p = target, value = map[p], length = 0, failed = 0;
    const uint32_t bound = value;
    if (value >= kGeoUnreached) { if (!lane) { out[0] = 0u; out[1] = 1u; } return; }      // (never: the host has looked at the target's word)
    for (uint32_t step = 0; step <= bound; ++step) {
        if (!lane && length < capacity) out[2u + length] = p;
        ++length;
        if (!value) break;
        const uint32_t row = p / N;
        const uint32_t q = lane < 27u ? geo_descent(map, N, p - row * N, row % N, row / N, lane, metric, value) : kGeoNone;
        const unsigned long long votes = __ballot(q != kGeoNone);
        if (!votes) { failed = 1u; break; }
        p = (uint32_t)__shfl((int)q, (int)__ffsll(votes) - 1);
        value = map[p];
    }
    if (!lane) { out[0] = length; out[1] = failed | (value ? 1u : 0u); }
}

static bool geo_valid(uint32_t N, int metric) { return N >= 1u && N <= kGeoMaxN && (metric == GEO_FACES || metric == GEO_CHAMFER) && geo_fits(N, metric); }

hipError_t launch_geodesic_init(const uint8_t* grid, uint32_t N, int of, int seedsKind, const void* seeds, uint32_t seedCount, uint32_t* map, const GeoScratch& l, hipStream_t s)
{
    if (!grid || !map || !l.flags[0] || N < 1u || N > kGeoMaxN || (of != GEO_SOLID && of != GEO_EMPTY) || seedsKind < GEO_SEEDS_BORDER || seedsKind > GEO_SEEDS_MASK ||
        (seedsKind != GEO_SEEDS_BORDER && !seeds && (seedsKind == GEO_SEEDS_MASK || seedCount)))
        return hipErrorInvalidValue;
    const size_t voxels = (size_t)N * N * N;
    const hipError_t e = hipMemsetAsync(l.flags[0], 0, l.flagBytes, s);
    if (e != hipSuccess) return e;
    k_geo_init<<<(uint32_t)((voxels + 255u) / 256u), 256, 0, s>>>(grid, N, of, seedsKind, seedsKind == GEO_SEEDS_MASK ? static_cast<const uint8_t*>(seeds) : nullptr, map, l.flags[0]);
    if (seedsKind == GEO_SEEDS_LIST && seedCount) k_geo_seed_list<<<(seedCount + 255u) / 256u, 256, 0, s>>>(static_cast<const uint32_t*>(seeds), seedCount, N, map, l.flags[0]);
    return hipGetLastError();
}

// One batch: `rounds` rounds, the first of them round `base` of the call (the flags a round reads are those of its number's parity), then the
// tally.  Control block and tally are cleared in front of the rounds.
hipError_t launch_geodesic_batch(uint32_t* map, uint32_t N, int metric, uint32_t limit, const GeoScratch& l, uint32_t rounds, uint32_t base, hipStream_t s)
{
    if (!map || !l.ctl || !l.flags[0] || !l.flags[1] || !l.queue || !geo_valid(N, metric)) return hipErrorInvalidValue;
    const uint32_t tiles = geo_tiles(N), voxels = N * N * N;
    if (rounds < 1u) rounds = 1u;
    if (rounds > kGeoMaxRounds) rounds = kGeoMaxRounds;
    const hipError_t e = hipMemsetAsync(l.ctl, 0, sizeof(GeoControl), s);
    if (e != hipSuccess) return e;
    const uint32_t blocks = tiles < kGeoRoundBlocks ? tiles : kGeoRoundBlocks;
    for (uint32_t k = 0; k < rounds; ++k) {
        uint8_t* cur = l.flags[(base + k) & 1u];
        uint8_t* next = l.flags[(base + k + 1u) & 1u];
        k_geo_compact<<<(tiles + 255u) / 256u, 256, 0, s>>>(cur, tiles, l.ctl, k, l.queue);
        if (metric == GEO_FACES) k_geo_round<GEO_FACES><<<blocks, 64, 0, s>>>(map, N, limit, l.ctl, k, l.queue, next);
        else k_geo_round<GEO_CHAMFER><<<blocks, 64, 0, s>>>(map, N, limit, l.ctl, k, l.queue, next);
    }
    const uint32_t want = (voxels + 255u) / 256u;
    k_geo_tally<<<want < kGeoTallyBlocks ? want : kGeoTallyBlocks, 256, 0, s>>>(map, voxels, l.ctl);
    return hipGetLastError();
}

// k_geo_compact for whoever keeps live flags, a queue and a control block of the same shape (access.hip)
hipError_t launch_geodesic_compact(uint8_t* live, uint32_t tiles, GeoControl* ctl, uint32_t round, uint32_t* queue, hipStream_t s)
{
    if (!live || !ctl || !queue || !tiles || round >= kGeoMaxRounds) return hipErrorInvalidValue;
    k_geo_compact<<<(tiles + 255u) / 256u, 256, 0, s>>>(live, tiles, ctl, round, queue);
    return hipGetLastError();
}

hipError_t launch_geodesic_path(const uint32_t* map, uint32_t N, int metric, uint32_t target, uint32_t* out, uint32_t capacity, hipStream_t s)
{
    if (!map || !out || !geo_valid(N, metric) || target >= N * N * N) return hipErrorInvalidValue;
    k_geo_path<<<1, 64, 0, s>>>(map, N, metric, target, out, capacity);
    return hipGetLastError();
}

} // namespace dxv
