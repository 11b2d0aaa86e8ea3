// partition.hip -- the maximal-ball partition of a whole N^3 grid into regions and throats (dxv_partition.h has the rule and the routines of every
// stage), on the frame's stream.  The caller waits once for {K, interface faces}, to size the table and the sort, and once for T, to size the
// throats; every other count stays in device memory.
//   field      distance.hip: F = DXV_DIST_SQ_I32 of the grid, into the operator's own buffer
//   keys       k_part_keys: F -> one 64-bit key per voxel, four voxels per thread; k_part_mip4, k_part_mip16: the maxima over 4^3 bricks and over
//              16^3 cells, one wave per cell, a lane per voxel (brick) of it
//   search     k_part_search: one wave per 4^3 brick, a lane per voxel of it as a centre: PartSearch, the argmax of the keys over the closed ball
//              pruned by the two mip levels (option partprune).  The lanes of a wave stand on neighbouring centres of radii a few units apart, so
//              they walk the same cells in the same order and their loads fall into the same lines.  parent goes where F was.
//   roots      k_part_walk: every member follows its parents to its root, reading parent, writing rootOf.  k_part_count, scan.hip's
//              launch_scan_sums, k_part_number: the roots -- rootOf[v] == v -- (and the interface faces, told by rootOf alone) per block of 1024
//              voxels, two counts in one word, the second above bit 16 (a thread's four items count at most 4 and 12, a block's 1024 and 3072);
//              the exclusive scan of the blocks; the roots' numbers by ascending index (where parent was)
//   regions    k_part_labels; k_part_stats: voxels, box and border bit by 32-bit atomics per region, once per wave where the wave's voxels are of
//              one region; k_part_table: the records
//   throats    k_part_emit_faces: one word (a, b) per interface face, by the same scan; radix_sort.hip; k_part_count_heads, launch_scan_sums: the
//              run heads = the unique pairs, T; then k_part_emit_pairs, k_part_face_atomics: every face finds its pair by binary search --
//              faces += 1, (neck, -voxel) = max as ONE 64-bit word --, k_part_throats: the records and the regions' throat counts
// No kernel waits for another workgroup, every loop is bounded, nothing goes to scratch memory.  Scratch and work are described once, by
// partition_carve and partition_work_carve (dxv_partition.h).
#include "dxv_device.h"
#include "dxv_partition.h"
#include "dxv_scan.h"

namespace dxv {

__global__ __launch_bounds__(256) void k_part_keys(const int32_t* __restrict__ F, uint32_t groups, int of, uint32_t cap, uint64_t* __restrict__ keys)
{
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    if (t >= groups) return;
    const int4 d = reinterpret_cast<const int4*>(F)[t];
    const uint32_t v = t * 4u;
    ulonglong2* out = reinterpret_cast<ulonglong2*>(keys + v);
    out[0] = make_ulonglong2(part_key(thick_radius(d.x, of, cap), v), part_key(thick_radius(d.y, of, cap), v + 1u));
    out[1] = make_ulonglong2(part_key(thick_radius(d.z, of, cap), v + 2u), part_key(thick_radius(d.w, of, cap), v + 3u));
}

__device__ __forceinline__ uint64_t part_wave_max(uint64_t k)
{
#pragma unroll
    for (uint32_t d = 1; d < 64u; d <<= 1) {
        const uint64_t o = __shfl_xor((unsigned long long)k, d);
        if (o > k) k = o;
    }
    return k;
}

// wave w of the launch: cell w of a level whose cells are 4^3 items of the level below (voxels: n = N; bricks: n = n4), a lane per item
__global__ __launch_bounds__(256) void k_part_mip(const uint64_t* __restrict__ below, uint32_t n, uint32_t cellsPerSide, uint64_t* __restrict__ mip)
{
    const uint32_t lane = threadIdx.x & 63u, cell = blockIdx.x * 4u + (threadIdx.x >> 6);
    if (cell >= cellsPerSide * cellsPerSide * cellsPerSide) return;     // (the whole wave)
    const uint32_t row = cell / cellsPerSide, bx = cell - row * cellsPerSide, by = row % cellsPerSide, bz = row / cellsPerSide;
    const uint32_t x = bx * 4u + (lane & 3u), y = by * 4u + ((lane >> 2) & 3u), z = bz * 4u + (lane >> 4);
    const uint64_t k = part_wave_max(x < n && y < n && z < n ? below[((size_t)z * n + y) * n + x] : 0ull);
    if (lane == 0u) mip[cell] = k;
}

// kCount: the measurement build of the same search (option partstages), which also counts the mip cells and the voxels it tests
template <bool kCount> __global__ __launch_bounds__(256) void k_part_search(PartParams p, uint32_t n4)
{
    const uint32_t lane = threadIdx.x & 63u, brick = blockIdx.x * 4u + (threadIdx.x >> 6), N = p.N;
    unsigned long long cells = 0, voxels = 0;
    if (brick < n4 * n4 * n4) {
        const uint32_t row = brick / n4, bx = brick - row * n4, by = row % n4, bz = row / n4;
        const uint32_t x = bx * 4u + (lane & 3u), y = by * 4u + ((lane >> 2) & 3u), z = bz * 4u + (lane >> 4);
        if (x < N && y < N && z < N) {
            const size_t v = ((size_t)z * N + y) * N + x;
            const uint32_t R = part_key_radius(p.keys[v]);
            uint32_t up = kPartNone;
            if (R) {
                PartSearch<kCount> s{p.keys, p.mip4, p.mip16, N, p.prune, x, y, z, R, 0ull, 0ull, 0ull};
                up = part_key_index(s.run());
                if (up >= N * N * N) up = (uint32_t)v;                  // (never: a key's index is a voxel of the grid)
                cells = s.cells; voxels = s.voxels;
            }
            p.parent[v] = up;
        }
    }
    if (!kCount) return;
#pragma unroll
    for (uint32_t d = 1; d < 64u; d <<= 1) { cells += __shfl_xor(cells, d); voxels += __shfl_xor(voxels, d); }
    if (lane == 0u && (cells || voxels)) {
        (void)__hip_atomic_fetch_add(p.counters, cells, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        (void)__hip_atomic_fetch_add(p.counters + 1, voxels, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

__global__ __launch_bounds__(256) void k_part_walk(const uint32_t* __restrict__ parent, uint32_t voxels, uint32_t* __restrict__ rootOf)
{
    const uint32_t v = blockIdx.x * 256u + threadIdx.x;
    if (v >= voxels) return;
    rootOf[v] = parent[v] == kPartNone ? kPartNone : part_root(parent, v, voxels);
}

// thread t of block b: voxels 1024 b + 4 t .. + 3 (N^3 is a multiple of 8: the four are all inside or all outside; a row may end after two of
// them, so the coordinates step).  The roots among them, and under kFaces their interface faces above bit 16
template <bool kFaces> __device__ __forceinline__ uint32_t part_count4(const uint32_t* __restrict__ id, uint32_t off, uint32_t N, uint32_t first, uint32_t voxels)
{
    if (first >= voxels) return 0u;
    const uint32_t row = first / N;
    uint32_t x = first - row * N, y = row % N, z = row / N, mine = 0;
#pragma unroll
    for (uint32_t k = 0; k < 4u; ++k) {
        if (id[first + k] == first + k) ++mine;
        if (kFaces) {
            uint32_t other[3];
            mine += part_popc3(part_faces(id, off, N, x, y, z, other)) << 16;
        }
        if (++x == N) { x = 0; if (++y == N) { y = 0; ++z; } }
    }
    return mine;
}

template <bool kFaces> __global__ __launch_bounds__(256) void k_part_count(const uint32_t* __restrict__ rootOf, uint32_t N, uint32_t voxels, unsigned long long* __restrict__ sums)
{
    uint32_t total;
    (void)block_scan_exclusive<uint32_t, 4>(part_count4<kFaces>(rootOf, kPartNone, N, blockIdx.x * kPartBlock + threadIdx.x * 4u, voxels), total);
    if (threadIdx.x == 0) { sums[2 * (size_t)blockIdx.x] = total & 0xffffu; sums[2 * (size_t)blockIdx.x + 1] = total >> 16; }
}

// the roots' numbers, 1 .. K by ascending index, at the roots' own voxels (the other words of `number` are never read)
__global__ __launch_bounds__(256) void k_part_number(const uint32_t* __restrict__ rootOf, uint32_t N, uint32_t voxels, const unsigned long long* __restrict__ sums,
                                                     uint32_t* __restrict__ number)
{
    const uint32_t first = blockIdx.x * kPartBlock + threadIdx.x * 4u;
    const uint32_t mine = part_count4<false>(rootOf, kPartNone, N, first, voxels);
    uint32_t total;
    uint32_t run = block_scan_exclusive<uint32_t, 4>(mine, total) + (uint32_t)sums[2 * (size_t)blockIdx.x];
    if (!mine) return;
#pragma unroll
    for (uint32_t k = 0; k < 4u; ++k)
        if (rootOf[first + k] == first + k) number[first + k] = ++run;
}

__global__ __launch_bounds__(256) void k_part_labels(const uint32_t* __restrict__ rootOf, const uint32_t* __restrict__ number, uint32_t voxels, uint32_t K,
                                                     uint32_t* __restrict__ labels)
{
    const uint32_t v = blockIdx.x * 256u + threadIdx.x;
    if (v >= voxels) return;
    const uint32_t r = rootOf[v];
    const uint32_t l = r < voxels ? number[r] : 0u;
    labels[v] = l <= K ? l : 0u;                                        // (never above K: the clamp keeps the atomics of the stats inside their table)
}

__global__ __launch_bounds__(256) void k_part_stats_init(PartStats* __restrict__ stats, uint32_t K)
{
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    if (t < K) stats[t] = part_stats_none();
}

__device__ __forceinline__ void part_stats_add(PartStats* s, uint32_t count, uint32_t x0, uint32_t x1, uint32_t y0, uint32_t y1, uint32_t z0, uint32_t z1, uint32_t flags)
{
    atomicAdd(&s->voxels, count);
    atomicMin(&s->lo[0], x0); atomicMin(&s->lo[1], y0); atomicMin(&s->lo[2], z0);
    atomicMax(&s->hi[0], x1); atomicMax(&s->hi[1], y1); atomicMax(&s->hi[2], z1);
    if (flags) atomicOr(&s->flags, flags);
}

// a thread per voxel; a wave whose 64 voxels are of one region sends its atomics once
__global__ __launch_bounds__(256) void k_part_stats(const uint32_t* __restrict__ labels, uint32_t N, uint32_t voxels, PartStats* __restrict__ stats)
{
    const uint32_t v = blockIdx.x * 256u + threadIdx.x, lane = threadIdx.x & 63u;
    const uint32_t l = v < voxels ? labels[v] : 0u;
    const uint32_t row = v / N, x = v - row * N, y = row % N, z = row / N;
    const uint32_t flags = part_border(x, y, z, N);
    const uint32_t first = (uint32_t)__builtin_amdgcn_readfirstlane((int)l);
    if (__all(l == first)) {
        if (!first) return;
        uint32_t x0 = x, x1 = x, y0 = y, y1 = y, z0 = z, z1 = z, f = flags;
#pragma unroll
        for (uint32_t d = 1; d < 64u; d <<= 1) {
            x0 = part_min(x0, (uint32_t)__shfl_xor((int)x0, d)); x1 = part_max(x1, (uint32_t)__shfl_xor((int)x1, d));
            y0 = part_min(y0, (uint32_t)__shfl_xor((int)y0, d)); y1 = part_max(y1, (uint32_t)__shfl_xor((int)y1, d));
            z0 = part_min(z0, (uint32_t)__shfl_xor((int)z0, d)); z1 = part_max(z1, (uint32_t)__shfl_xor((int)z1, d));
            f |= (uint32_t)__shfl_xor((int)f, d);
        }
        if (lane == 0u) part_stats_add(stats + (first - 1u), 64u, x0, x1, y0, y1, z0, z1, f);
    } else if (l) {
        part_stats_add(stats + (l - 1u), 1u, x, x, y, y, z, z, flags);
    }
}

__global__ __launch_bounds__(256) void k_part_table(const uint32_t* __restrict__ rootOf, const uint32_t* __restrict__ number, const uint64_t* __restrict__ keys, uint32_t voxels,
                                                    uint32_t K, const PartStats* __restrict__ stats, PartRegion* __restrict__ table)
{
    const uint32_t v = blockIdx.x * 256u + threadIdx.x;
    if (v >= voxels || rootOf[v] != v) return;
    const uint32_t i = number[v] - 1u;
    if (i < K) table[i] = part_region(v, part_key_radius(keys[v]), stats[i]);
}

// one word per interface face, in the order of the voxels: the scan of k_part_count<true>, redone on the labels (a face is an interface face
// under the labels exactly when it is one under the roots)
__global__ __launch_bounds__(256) void k_part_emit_faces(const uint32_t* __restrict__ labels, uint32_t N, uint32_t voxels, const unsigned long long* __restrict__ sums,
                                                         uint32_t shift, unsigned long long total, uint64_t* __restrict__ out)
{
    const uint32_t first = blockIdx.x * kPartBlock + threadIdx.x * 4u;
    uint32_t bits[4] = {0u, 0u, 0u, 0u}, other[4][3], mine = 0;
    if (first < voxels) {
        const uint32_t row = first / N;
        uint32_t x = first - row * N, y = row % N, z = row / N;
#pragma unroll
        for (uint32_t k = 0; k < 4u; ++k) {
            bits[k] = part_faces(labels, 0u, N, x, y, z, other[k]);
            mine += part_popc3(bits[k]);
            if (++x == N) { x = 0; if (++y == N) { y = 0; ++z; } }
        }
    }
    uint32_t blockTotal;
    unsigned long long at = sums[2 * (size_t)blockIdx.x + 1] + block_scan_exclusive<uint32_t, 4>(mine, blockTotal);
    if (!mine) return;
#pragma unroll
    for (uint32_t k = 0; k < 4u; ++k)
#pragma unroll
        for (uint32_t e = 0; e < 3u; ++e)
            if (bits[k] >> e & 1u) {
                if (at < total) out[at] = part_pair(labels[first + k], other[k][e], shift);    // (always: both scans count the same faces)
                ++at;
            }
}

// thread t of block b: sorted words 1024 b + 4 t .. + 3; a head is a word that differs from the one in front of it
__device__ __forceinline__ uint32_t part_heads4(const uint64_t* __restrict__ sorted, uint32_t n, uint32_t first)
{
    uint32_t heads = 0;
#pragma unroll
    for (uint32_t k = 0; k < 4u; ++k) {
        const uint32_t i = first + k;
        if (i < n && (i == 0u || sorted[i] != sorted[i - 1u])) heads |= 1u << k;
    }
    return heads;
}
__global__ __launch_bounds__(256) void k_part_count_heads(const uint64_t* __restrict__ sorted, uint32_t n, unsigned long long* __restrict__ sums)
{
    uint32_t total;
    (void)block_scan_exclusive<uint32_t, 4>((uint32_t)__popc(part_heads4(sorted, n, blockIdx.x * kPartBlock + threadIdx.x * 4u)), total);
    if (threadIdx.x == 0) { sums[2 * (size_t)blockIdx.x] = total; sums[2 * (size_t)blockIdx.x + 1] = 0; }
}
__global__ __launch_bounds__(256) void k_part_emit_pairs(const uint64_t* __restrict__ sorted, uint32_t n, const unsigned long long* __restrict__ sums, uint32_t T,
                                                         uint64_t* __restrict__ pairs)
{
    const uint32_t first = blockIdx.x * kPartBlock + threadIdx.x * 4u;
    const uint32_t heads = part_heads4(sorted, n, first);
    uint32_t total;
    uint32_t at = (uint32_t)sums[2 * (size_t)blockIdx.x] + block_scan_exclusive<uint32_t, 4>((uint32_t)__popc(heads), total);
    if (!heads) return;
#pragma unroll
    for (uint32_t k = 0; k < 4u; ++k)
        if (heads >> k & 1u) {
            if (at < T) pairs[at] = sorted[first + k];
            ++at;
        }
}

__global__ __launch_bounds__(256) void k_part_face_atomics(const uint32_t* __restrict__ labels, const uint64_t* __restrict__ keys, uint32_t N, uint32_t voxels,
                                                           const uint64_t* __restrict__ pairs, uint32_t T, uint32_t shift, uint32_t* __restrict__ count,
                                                           unsigned long long* __restrict__ neck)
{
    const uint32_t v = blockIdx.x * 256u + threadIdx.x;
    if (v >= voxels) return;
    const uint32_t row = v / N, x = v - row * N, y = row % N, z = row / N;
    uint32_t other[3];
    const uint32_t bits = part_faces(labels, 0u, N, x, y, z, other);
    if (!bits) return;
    const uint32_t mine = labels[v], R = part_key_radius(keys[v]);
    const uint32_t step[3] = {1u, N, N * N};
#pragma unroll
    for (uint32_t e = 0; e < 3u; ++e) {
        if (!(bits >> e & 1u)) continue;
        const uint32_t t = part_find_pair(pairs, T, part_pair(mine, other[e], shift));
        if (t >= T) continue;                                           // (never: every face's pair is among the unique ones)
        atomicAdd(count + t, 1u);
        (void)__hip_atomic_fetch_max(neck + t, (unsigned long long)part_neck_word(part_min(R, part_key_radius(keys[v + step[e]])), v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

__global__ __launch_bounds__(256) void k_part_throats(const uint64_t* __restrict__ pairs, const uint32_t* __restrict__ count, const unsigned long long* __restrict__ neck, uint32_t T,
                                                      uint32_t shift, uint32_t K, uint32_t* __restrict__ throats, PartRegion* __restrict__ table)
{
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    if (t >= T) return;
    const PartThroat r = part_throat(pairs[t], shift, count[t], neck[t]);
    uint32_t* out = throats + 5u * (size_t)t;
    out[0] = r.a; out[1] = r.b; out[2] = r.faces; out[3] = r.neck_sq; out[4] = r.neck_voxel;
    if (r.a - 1u < K) atomicAdd(&table[r.a - 1u].throats, 1u);
    if (r.b - 1u < K) atomicAdd(&table[r.b - 1u].throats, 1u);
}

static bool part_valid(const uint8_t* grid, const PartParams& p)
{
    return grid && p.F && p.N >= 2u && p.N <= kThickMaxN && !(p.N & 1u) && (p.of == PART_SOLID || p.of == PART_EMPTY) && p.cap >= kPartMinCapSq && p.cap <= kPartMaxCapSq &&
           p.prune <= 3u;
}

hipError_t launch_partition_stage(const uint8_t* grid, const PartParams& p, int stage, hipStream_t s)
{
    if (!part_valid(grid, p)) return hipErrorInvalidValue;
    const uint32_t N = p.N, voxels = N * N * N, groups = voxels / 4u, blocks = part_blocks(voxels), perVoxel = (voxels + 255u) / 256u;
    const uint32_t n4 = part_cells(N, 4u), n16 = part_cells(N, 16u);
    hipError_t e = hipSuccess;
    switch (stage) {
    case PART_STAGE_FIELD:
        return launch_distance(grid, N, 0, p.F, p.passes, s);
    case PART_STAGE_KEYS:
        k_part_keys<<<(groups + 255u) / 256u, 256, 0, s>>>(p.F, groups, p.of, p.cap, p.keys);
        k_part_mip<<<(n4 * n4 * n4 + 3u) / 4u, 256, 0, s>>>(p.keys, N, n4, p.mip4);
        k_part_mip<<<(n16 * n16 * n16 + 3u) / 4u, 256, 0, s>>>(p.mip4, n4, n16, p.mip16);
        break;
    case PART_STAGE_SEARCH:
        if ((e = hipMemsetAsync(p.counters, 0, 2u * sizeof(unsigned long long), s)) != hipSuccess) return e;
        if (p.count) k_part_search<true><<<(n4 * n4 * n4 + 3u) / 4u, 256, 0, s>>>(p, n4);
        else k_part_search<false><<<(n4 * n4 * n4 + 3u) / 4u, 256, 0, s>>>(p, n4);
        break;
    case PART_STAGE_ROOTS:
        k_part_walk<<<perVoxel, 256, 0, s>>>(p.parent, voxels, p.rootOf);
        if (p.wantThroats) k_part_count<true><<<blocks, 256, 0, s>>>(p.rootOf, N, voxels, p.sums);
        else k_part_count<false><<<blocks, 256, 0, s>>>(p.rootOf, N, voxels, p.sums);
        if ((e = launch_scan_sums(p.sums, 2, blocks, p.sums + 2 * (size_t)blocks, s)) != hipSuccess) return e;
        k_part_number<<<blocks, 256, 0, s>>>(p.rootOf, N, voxels, p.sums, p.number);
        break;
    case PART_STAGE_REGIONS:                                            // (behind the caller's wait for the totals: labels, table and work are in place)
        if (!p.labels || (p.K && (!p.table || !p.stats))) return hipErrorInvalidValue;
        k_part_labels<<<perVoxel, 256, 0, s>>>(p.rootOf, p.number, voxels, p.K, p.labels);
        if (!p.K) break;
        k_part_stats_init<<<(p.K + 255u) / 256u, 256, 0, s>>>(p.stats, p.K);
        k_part_stats<<<perVoxel, 256, 0, s>>>(p.labels, N, voxels, p.stats);
        k_part_table<<<perVoxel, 256, 0, s>>>(p.rootOf, p.number, p.keys, voxels, p.K, p.stats, p.table);
        break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

// the throats' first half: the faces' words, sorted, and the count of their run heads -- T, at p.pairTotal -- for the caller to wait for
hipError_t launch_partition_pairs(PartParams& p, hipStream_t s)
{
    if (!p.faces || p.faces > 0xFFFFFFFFull || !p.K || !p.labels || !p.sortA) return hipErrorInvalidValue;
    const uint32_t N = p.N, voxels = N * N * N, n = (uint32_t)p.faces, shift = part_label_bits(p.K);
    k_part_emit_faces<<<part_blocks(voxels), 256, 0, s>>>(p.labels, N, voxels, p.sums, shift, p.faces, p.sortA);
    uint64_t* sorted = nullptr;
    const hipError_t e = radix_sort_keys_bits(p.sortA, p.sortB, n, p.hist, 0, (int)(2u * shift), &sorted, s, -1);
    if (e != hipSuccess) return e;
    p.sorted = sorted;
    p.pairs = sorted == p.sortA ? p.sortB : p.sortA;
    k_part_count_heads<<<part_blocks(n), 256, 0, s>>>(p.sorted, n, p.headSums);
    return launch_scan_sums(p.headSums, 2, part_blocks(n), p.headSums + 2 * (size_t)part_blocks(n), s);
}
// ... and their second, with T known and `throats` (20 T bytes) in place
hipError_t launch_partition_throats(const PartParams& p, uint32_t T, uint32_t* throats, hipStream_t s)
{
    if (!T || T > p.faces || !throats || !p.sorted || !p.pairs || !p.table) return hipErrorInvalidValue;
    const uint32_t N = p.N, voxels = N * N * N, n = (uint32_t)p.faces, shift = part_label_bits(p.K);
    k_part_emit_pairs<<<part_blocks(n), 256, 0, s>>>(p.sorted, n, p.headSums, T, p.pairs);
    unsigned long long* neck = reinterpret_cast<unsigned long long*>(p.sorted);    // (the sorted words have been read)
    hipError_t e = hipMemsetAsync(neck, 0, (size_t)T * sizeof(unsigned long long), s);
    if (e == hipSuccess) e = hipMemsetAsync(p.pairCount, 0, (size_t)T * sizeof(uint32_t), s);
    if (e != hipSuccess) return e;
    k_part_face_atomics<<<(voxels + 255u) / 256u, 256, 0, s>>>(p.labels, p.keys, N, voxels, p.pairs, T, shift, p.pairCount, neck);
    k_part_throats<<<(T + 255u) / 256u, 256, 0, s>>>(p.pairs, p.pairCount, neck, T, shift, p.K, throats, p.table);
    return hipGetLastError();
}

} // namespace dxv
