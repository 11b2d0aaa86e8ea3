// access.hip -- the access radius inside a whole N^3 grid, and what its intrusion map needs (dxv_access.h has the rule and the routines), on the
// frame's stream:
//   field             distance.hip: F = DXV_DIST_SQ_I32 of the grid, into the operator's own scratch; R = thick_radius(F)
//   k_acc_init        F and the seeds -> A's first words (R on a seed that is a member, 0 elsewhere), the live flags of round 0 -- every tile that
//                     holds a seed or a neighbour of one -- and the number of seeds used
//   k_acc_seed_list   ... the seeds of a list, behind an init without seeds; a duplicate finds the word raised and counts nothing
//   k_geo_compact     geodesic.hip's, as it is: a round's live flags -> its queue of tiles and their number (word `round` of the control block)
//   k_acc_round       a wave per queued tile, tiles dealt in a bounded grid-stride loop: A of the tile and its halo from the map into LDS (10^3
//                     words), R of the lane's z column into eight registers, swept there until a wave-wide vote says nothing rose, the words
//                     that rose back into the map, and in the NEXT round's flags every neighbour tile that borders one of them
//   k_acc_tally       A and F -> reached, unreached, the widest voxel; the seeds used ride along
//   k_acc_radius      A -> F in thick_radius's encoding, once A has settled: thickness.hip's stages paint the intrusion map from it
// The histograms are thickness.hip's k_thick_histogram (launch_thickness_stage).
// A batch is `rounds` rounds behind one another.  The kernels of a round return at once when the round before left nothing live, so a batch
// costs what its live rounds cost, and the host reads the block where the frame is next synchronised (dxv_products.hip: settle_access).
// Stale reads.  A tile reads its neighbours' words while they may be raising them.  Words only rise, and every word ever stored is the least
// radius along a real path of members from a seed: a stale word is a valid lower bound, and whoever raises a word on a tile's border flags the
// tiles beyond it for the next round, so the chain stops only at a fixed point.  The fixed point reached from this start is unique: no word
// exceeds A (each is a real path's), and at a fixed point none is below it (induction along a best path).  Of the voxels whose word is not
// final yet, the one with the highest A whose path predecessor is final becomes final in the next round that runs its tile -- and that tile is
// flagged, by the round that made the predecessor final or by the seeds --, so V live rounds bound the call.
// No workgroup waits for another, every loop is bounded, launch sizes depend on N alone; no scratch memory.  The flood's blocks and, behind them,
// the field's or the whole thickness's are laid out by access_carve (dxv_access.h).
#include "dxv_device.h"
#include "dxv_access.h"

namespace dxv {

constexpr uint32_t kAccRoundBlocks = 8192;        // workgroups (of one wave) a round is launched with at the most, whatever its queue holds
constexpr uint32_t kAccTallyBlocks = 1024;        // ... the tally, of four waves

// one thread per voxel; a wave counts its seeds with one atomic
__global__ __launch_bounds__(256) void k_acc_init(const int32_t* __restrict__ F, uint32_t N, int of, uint32_t cap, int seedsKind, const uint8_t* __restrict__ seedMask,
                                                  uint32_t* __restrict__ A, uint8_t* __restrict__ live, unsigned long long* __restrict__ seedsUsed)
{
    const size_t v = (size_t)blockIdx.x * 256u + threadIdx.x;
    bool used = false;
    if (v < (size_t)N * N * N) {
        const uint32_t row = (uint32_t)(v / N), x = (uint32_t)(v - (size_t)row * N), y = row % N, z = row / N;
        const bool seed = seedsKind == GEO_SEEDS_BORDER ? geo_border(x, y, z, N) : seedsKind == GEO_SEEDS_MASK ? seedMask[v] != 0 : false;
        const uint32_t word = acc_start(thick_radius(F[v], of, cap), seed);
        A[v] = word;
        used = word != 0u;
        if (used) geo_mark_seed(live, geo_tiles_side(N), x, y, z);      // (the same byte from every seed of a tile)
    }
    const unsigned long long votes = __ballot(used);
    if (votes && (threadIdx.x & 63u) == (uint32_t)__ffsll(votes) - 1u)
        (void)__hip_atomic_fetch_add(seedsUsed, (unsigned long long)__popcll(votes), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// one thread per entry of the list; of the duplicates of a voxel one finds its word at 0 and counts it
__global__ __launch_bounds__(256) void k_acc_seed_list(const uint32_t* __restrict__ seeds, uint32_t count, const int32_t* __restrict__ F, uint32_t N, int of, uint32_t cap,
                                                       uint32_t* __restrict__ A, uint8_t* __restrict__ live, unsigned long long* __restrict__ seedsUsed)
{
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    if (t >= count) return;
    const uint32_t v = seeds[t];
    if (v >= N * N * N) return;                                         // (the host has refused an index outside the grid)
    const uint32_t R = thick_radius(F[v], of, cap);
    if (!R) return;                                                     // (a seed that is no member is ignored)
    const uint32_t row = v / N;
    if (atomicMax(A + v, R) == 0u) (void)__hip_atomic_fetch_add(seedsUsed, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    geo_mark_seed(live, geo_tiles_side(N), v - row * N, row % N, row / N);
}

// One wave per tile.  Lane (ly, lx) owns the column of eight voxels along z, as in k_geo_round: a b32 access of the wave then touches banks
// 10 ly + lx + const, which are distinct within each half of the wave (0 .. 37 and 40 .. 77 mod 64).
template <int kConnectivity> __global__ __launch_bounds__(64) void k_acc_round(uint32_t* A, const int32_t* __restrict__ F, uint32_t N, int of, uint32_t cap,
                                                                               const GeoControl* __restrict__ ctl, uint32_t round, const uint32_t* __restrict__ queue,
                                                                               uint8_t* __restrict__ next)
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
            T[w] = v != kGeoNone ? A[v] : 0u;
        }
        uint32_t R[kGeoTile];
#pragma unroll
        for (uint32_t z = 0; z < kGeoTile; ++z) {
            const uint32_t v = geo_tile_voxel(tx, ty, tz, geo_tile_at(lx, ly, z), N);
            R[z] = v != kGeoNone ? thick_radius(F[v], of, cap) : 0u;
        }
        __syncthreads();
        uint32_t orig[kGeoTile];
#pragma unroll
        for (uint32_t z = 0; z < kGeoTile; ++z) orig[z] = T[geo_tile_at(lx, ly, z)];
        bool unsettled = true;
        for (uint32_t sweep = 0; sweep < kAccMaxSweeps; ++sweep) {
            bool rose = false;
#pragma unroll
            for (uint32_t z = 0; z < kGeoTile; ++z) {
                const uint32_t at = geo_tile_at(lx, ly, z), cur = T[at], v = acc_relax<kConnectivity>(T, at, cur, R[z]);
                if (v != cur) { T[at] = v; rose = true; }
            }
            __syncthreads();
            if (!__any(rose)) { unsettled = false; break; }
        }
        uint32_t mask = unsettled ? 1u << kGeoSelf : 0u;                // (never: the sweeps' bound is the relaxation's own; then the tile runs again)
#pragma unroll
        for (uint32_t z = 0; z < kGeoTile; ++z) {
            const uint32_t v = T[geo_tile_at(lx, ly, z)];
            if (v == orig[z]) continue;
            A[geo_tile_voxel(tx, ty, tz, geo_tile_at(lx, ly, z), N)] = v;       // (a word that rose is a member's, R > 0: inside the grid)
            mask |= acc_touch(lx, ly, z, kConnectivity);
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

__global__ __launch_bounds__(256) void k_acc_tally(const uint32_t* __restrict__ A, const int32_t* __restrict__ F, uint32_t voxels, int of, uint32_t cap,
                                                   const unsigned long long* __restrict__ seedsUsed, GeoControl* __restrict__ ctl)
{
    __shared__ AccTally part[4];
    AccTally t{0, 0, 0, 0};
    if (blockIdx.x == 0u && threadIdx.x == 0u) t.seeds = *seedsUsed;
    for (uint32_t v = blockIdx.x * 256u + threadIdx.x; v < voxels; v += gridDim.x * 256u) acc_tally_voxel(t, A[v], thick_radius(F[v], of, cap), v);
#pragma unroll
    for (uint32_t d = 1; d < 64u; d <<= 1) {
        const AccTally o{__shfl_xor(t.seeds, d), __shfl_xor(t.reached, d), __shfl_xor(t.unreached, d), __shfl_xor(t.key, d)};
        acc_tally_combine(t, o);
    }
    if ((threadIdx.x & 63u) == 0u) part[threadIdx.x >> 6] = t;
    __syncthreads();
    if (threadIdx.x) return;
    for (uint32_t k = 1; k < 4u; ++k) acc_tally_combine(t, part[k]);
    if (t.seeds) (void)__hip_atomic_fetch_add(&ctl->tally[0], t.seeds, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (t.reached) (void)__hip_atomic_fetch_add(&ctl->tally[1], t.reached, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (t.unreached) (void)__hip_atomic_fetch_add(&ctl->tally[2], t.unreached, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (t.key) (void)__hip_atomic_fetch_max(&ctl->tally[3], t.key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// four voxels per thread (N is even: N^3 is a multiple of 8)
__global__ __launch_bounds__(256) void k_acc_radius(const uint32_t* __restrict__ A, uint32_t groups, int of, int32_t* __restrict__ F)
{
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    if (t >= groups) return;
    const uint4 a = reinterpret_cast<const uint4*>(A)[t];
    reinterpret_cast<int4*>(F)[t] = make_int4(acc_radius_word(a.x, of), acc_radius_word(a.y, of), acc_radius_word(a.z, of), acc_radius_word(a.w, of));
}

hipError_t launch_access_init(const uint8_t* grid, uint32_t N, int of, uint32_t cap, int seedsKind, const void* seeds, uint32_t seedCount, uint32_t* A, const AccScratch& l, hipStream_t s)
{
    if (!grid || !A || !l.seedsUsed || !l.flags[0] || !l.thick.F || !l.thick.passes || !acc_valid(N, of, 6, cap) || seedsKind < GEO_SEEDS_BORDER || seedsKind > GEO_SEEDS_MASK ||
        (seedsKind != GEO_SEEDS_BORDER && !seeds && (seedsKind == GEO_SEEDS_MASK || seedCount)))
        return hipErrorInvalidValue;
    const ThickParams& p = l.thick;
    const size_t voxels = (size_t)N * N * N;
    hipError_t e = launch_distance(grid, N, 0, p.F, p.passes, s);
    if (e != hipSuccess) return e;
    if ((e = hipMemsetAsync(l.seedsUsed, 0, l.clearBytes, s)) != hipSuccess) return e;     // (the seeds' word and both sets of flags)
    k_acc_init<<<(uint32_t)((voxels + 255u) / 256u), 256, 0, s>>>(p.F, N, of, cap, seedsKind, seedsKind == GEO_SEEDS_MASK ? static_cast<const uint8_t*>(seeds) : nullptr, A, l.flags[0],
                                                                  l.seedsUsed);
    if (seedsKind == GEO_SEEDS_LIST && seedCount)
        k_acc_seed_list<<<(seedCount + 255u) / 256u, 256, 0, s>>>(static_cast<const uint32_t*>(seeds), seedCount, p.F, N, of, cap, A, l.flags[0], l.seedsUsed);
    return hipGetLastError();
}

// One batch: `rounds` rounds, the first of them round `base` of the call (the flags a round reads are those of its number's parity), then the
// tally.  Control block and tally are cleared in front of the rounds.
hipError_t launch_access_batch(uint32_t* A, uint32_t N, int of, int connectivity, uint32_t cap, const AccScratch& l, uint32_t rounds, uint32_t base, hipStream_t s)
{
    if (!A || !l.ctl || !l.flags[0] || !l.flags[1] || !l.queue || !l.thick.F || !acc_valid(N, of, connectivity, cap)) return hipErrorInvalidValue;
    const ThickParams& p = l.thick;
    const uint32_t tiles = geo_tiles(N), voxels = N * N * N;
    if (rounds < 1u) rounds = 1u;
    if (rounds > kAccMaxRounds) rounds = kAccMaxRounds;
    hipError_t e = hipMemsetAsync(l.ctl, 0, sizeof(GeoControl), s);
    if (e != hipSuccess) return e;
    const uint32_t blocks = tiles < kAccRoundBlocks ? tiles : kAccRoundBlocks;
    for (uint32_t k = 0; k < rounds; ++k) {
        uint8_t* cur = l.flags[(base + k) & 1u];
        uint8_t* next = l.flags[(base + k + 1u) & 1u];
        if ((e = launch_geodesic_compact(cur, tiles, l.ctl, k, l.queue, s)) != hipSuccess) return e;
        if (connectivity == 6) k_acc_round<6><<<blocks, 64, 0, s>>>(A, p.F, N, of, cap, l.ctl, k, l.queue, next);
        else k_acc_round<26><<<blocks, 64, 0, s>>>(A, p.F, N, of, cap, l.ctl, k, l.queue, next);
    }
    const uint32_t want = (voxels + 255u) / 256u;
    k_acc_tally<<<want < kAccTallyBlocks ? want : kAccTallyBlocks, 256, 0, s>>>(A, p.F, voxels, of, cap, l.seedsUsed, l.ctl);
    return hipGetLastError();
}

hipError_t launch_access_radius(const uint32_t* A, uint32_t N, int of, const AccScratch& l, hipStream_t s)
{
    if (!A || !l.thick.F || !acc_valid(N, of, 6, kThickMinCapSq)) return hipErrorInvalidValue;
    const uint32_t groups = N * N * N / 4u;
    k_acc_radius<<<(groups + 255u) / 256u, 256, 0, s>>>(A, groups, of, l.thick.F);
    return hipGetLastError();
}

} // namespace dxv
