// skeleton.hip -- the skeleton graph of a whole N^3 grid (dxv_skeleton.h has the rule's routines), on the frame's stream.  One pass over the mask
// per step, no fixed-point rounds:
//   (k_comp_pack)      grid -> the member mask, components.hip's (launch_comp_pack)
//   k_skel_classify    one lane per mask word: the nine words of its column of rows first; a word without a member ends there.  Otherwise the
//                      eighteen words beside them for their carry bits, the 26 planes into the saturating counter (skel_classify), the node, curve
//                      and end words stored, and the wave's three popcounts sent by one lane.  The three masks are cleared in front of it.
//   k_skel_init        parent[p] = the start of p's run inside its own word of the node mask or of the curve mask, kCompNone for a non-member
//   (k_comp_merge, k_comp_compress)   components.hip's, once over the node mask and once over the curve mask at connectivity 26, then the
//                      roots (launch_comp_merge, launch_comp_compress); DESIGN §4.10's argument for their loops applies unchanged: a union joins
//                      two voxels of ONE mask, the masks are disjoint, so an entry only ever points into its own node or branch
//   k_skel_roots       a wave per 64 voxels in linear order: the node roots and the curve roots as bits, and their two counts
//   scan.hip           the exclusive scan of the count pairs (launch_scan_words, C = 2); the totals {K, B} are what the host reads
//   k_skel_number      labels[p] = rank of p's root among its kind's roots + 1, with bit 31 for a branch; in place
//   k_skel_stats_init, k_skel_first, k_skel_stats, k_skel_nodes, k_skel_branches
//                      behind the host's read of K and B: `first` from the root bits; one lane per mask word gathers a set of sums, minima, maxima
//                      and ORs per run of node voxels and per run of curve voxels (one label each) and sends it with integer atomics; the steps
//                      and attachments of every curve voxel from its neighbours (skel_neighbours); then the records, nodes before branches
//   k_skel_prune_mark, k_skel_prune_edit
//                      dxv_skeleton_prune: a flag per branch and per tip from the tables, two counters; one pass over labels and grid
// Every loop is bounded by the bits of a word or by the 26 neighbours; no kernel here uses scratch memory or LDS, none waits for another workgroup.
#include "dxv_device.h"
#include "dxv_skeleton.h"

namespace dxv {

__global__ __launch_bounds__(256) void k_skel_classify(const uint64_t* __restrict__ member, uint32_t N, uint64_t* __restrict__ node, uint64_t* __restrict__ curve,
                                                       uint64_t* __restrict__ ends, unsigned long long* counters, uint32_t words)
{
    const uint32_t t = blockIdx.x * 256u + threadIdx.x, lane = threadIdx.x & 63u;
    const uint32_t W = fill_row_words(N);
    const uint32_t row = t < words ? t / W : 0u, w = t < words ? t - row * W : 0u;
    const int iy = (int)(row % N), iz = (int)(row / N);
    SkelRow rows[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) {                                       // the nine loads, issued together
        const int ny = iy + k % 3 - 1, nz = iz + k / 3 - 1;
        const bool in = t < words && ny >= 0 && ny < (int)N && nz >= 0 && nz < (int)N;
        rows[k].cur = in ? member[((size_t)nz * N + (size_t)ny) * W + w] : 0ull;
        rows[k].prev = 0ull; rows[k].next = 0ull;
    }
    const bool live = rows[4].cur != 0ull;
    if (!__any(live)) return;                                           // (the whole wave)
    uint32_t nEnds = 0, nCurve = 0, nJunctions = 0;
    if (live) {
#pragma unroll
        for (int k = 0; k < 9; ++k) {
            const int ny = iy + k % 3 - 1, nz = iz + k / 3 - 1;
            if (ny < 0 || ny >= (int)N || nz < 0 || nz >= (int)N) continue;
            const uint64_t* at = member + ((size_t)nz * N + (size_t)ny) * W + w;
            if (w) rows[k].prev = at[-1];
            if (w + 1u < W) rows[k].next = at[1];
        }
        const SkelClass c = skel_classify(rows);
        node[t] = c.node; curve[t] = c.curve; ends[t] = c.ends;
        nEnds = comp_popc(c.ends); nCurve = comp_popc(c.curve); nJunctions = comp_popc(c.junctions);
    }
#pragma unroll
    for (uint32_t d = 1; d < 64u; d <<= 1) {                            // (every lane of the wave is here)
        nEnds += (uint32_t)__shfl_xor((int)nEnds, (int)d);
        nCurve += (uint32_t)__shfl_xor((int)nCurve, (int)d);
        nJunctions += (uint32_t)__shfl_xor((int)nJunctions, (int)d);
    }
    if (lane == 0u) {
        if (nEnds) (void)__hip_atomic_fetch_add(counters + 0, (unsigned long long)nEnds, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (nCurve) (void)__hip_atomic_fetch_add(counters + 1, (unsigned long long)nCurve, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (nJunctions) (void)__hip_atomic_fetch_add(counters + 2, (unsigned long long)nJunctions, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// four consecutive voxels per thread (N is even: N^3 is a multiple of 8)
__global__ __launch_bounds__(256) void k_skel_init(const uint64_t* __restrict__ node, const uint64_t* __restrict__ curve, uint32_t N, uint32_t* __restrict__ parent, uint32_t total)
{
    const size_t first = ((size_t)blockIdx.x * 256u + threadIdx.x) * 4u;
    if (first >= total) return;
    const uint32_t p = (uint32_t)first;
    *reinterpret_cast<uint4*>(parent + p) = make_uint4(skel_init_parent(node, curve, N, p), skel_init_parent(node, curve, N, p + 1u), skel_init_parent(node, curve, N, p + 2u),
                                                       skel_init_parent(node, curve, N, p + 3u));
}

// a wave per 64 voxels in linear order
__global__ __launch_bounds__(256) void k_skel_roots(const uint32_t* __restrict__ parent, const uint64_t* __restrict__ curve, uint32_t N, uint32_t total,
                                                    uint64_t* __restrict__ nodeRoots, uint64_t* __restrict__ curveRoots, uint32_t* __restrict__ counts, uint32_t words)
{
    const uint32_t word = blockIdx.x * 4u + (threadIdx.x >> 6);
    if (word >= words) return;                                          // (the whole wave)
    const uint32_t lane = threadIdx.x & 63u;
    const size_t p = (size_t)word * 64u + lane;
    const bool root = p < total && parent[p] == (uint32_t)p;
    const bool ofCurve = root && skel_bit(curve, N, (uint32_t)p);
    const uint64_t nr = __ballot(root && !ofCurve), cr = __ballot(ofCurve);
    if (lane == 0u) {
        nodeRoots[word] = nr; curveRoots[word] = cr;
        counts[2u * word] = comp_popc(nr); counts[2u * word + 1u] = comp_popc(cr);
    }
}

__device__ __forceinline__ uint32_t skel_label_of(uint32_t root, const uint64_t* __restrict__ nodeRoots, const uint64_t* __restrict__ curveRoots, const uint32_t* __restrict__ counts)
{
    if (root == kCompNone) return 0u;
    const uint32_t word = root >> 6;
    const uint64_t below = (1ull << (root & 63u)) - 1ull, cr = curveRoots[word];
    const bool branch = (cr >> (root & 63u) & 1ull) != 0ull;
    const uint32_t rank = branch ? counts[2u * word + 1u] + comp_popc(cr & below) : counts[2u * word] + comp_popc(nodeRoots[word] & below);
    return skel_label(rank + 1u, branch);
}
// four consecutive voxels per thread
__global__ __launch_bounds__(256) void k_skel_number(uint32_t* labels, uint32_t total, const uint64_t* __restrict__ nodeRoots, const uint64_t* __restrict__ curveRoots,
                                                     const uint32_t* __restrict__ counts)
{
    const size_t first = ((size_t)blockIdx.x * 256u + threadIdx.x) * 4u;
    if (first >= total) return;
    uint4* at = reinterpret_cast<uint4*>(labels + first);
    const uint4 r = *at;
    *at = make_uint4(skel_label_of(r.x, nodeRoots, curveRoots, counts), skel_label_of(r.y, nodeRoots, curveRoots, counts), skel_label_of(r.z, nodeRoots, curveRoots, counts),
                     skel_label_of(r.w, nodeRoots, curveRoots, counts));
}

__global__ __launch_bounds__(256) void k_skel_stats_init(SkelNodeStats* __restrict__ stats, uint32_t K, SkelBranch* __restrict__ branches, uint32_t B)
{
    const uint32_t k = blockIdx.x * 256u + threadIdx.x;
    if (k < K) {
        SkelNodeStats s;
        s.voxels = 0u; s.degree = 0u; s.flags = 0u; s.w_max = 0u;
        for (int a = 0; a < 3; ++a) { s.lo[a] = 0xffffffffu; s.hi[a] = 0u; }
        stats[k] = s;
    }
    if (k < B) {
        SkelBranch r;
        r.a = kCompNone; r.b = 0u; r.first = 0u; r.voxels = 0u; r.steps[0] = r.steps[1] = r.steps[2] = 0u; r.flags = 0u;
        r.w_min = 0xffffffffu; r.w_max = 0u; r.w_sum = 0ull;
        branches[k] = r;
    }
}

// one lane per 64 voxels in linear order: the roots among them are the `first` of consecutive nodes and of consecutive branches
__global__ __launch_bounds__(256) void k_skel_first(const uint64_t* __restrict__ nodeRoots, const uint64_t* __restrict__ curveRoots, const uint32_t* __restrict__ counts,
                                                    uint32_t words, SkelNode* __restrict__ nodes, uint32_t K, SkelBranch* __restrict__ branches, uint32_t B)
{
    const uint32_t word = blockIdx.x * 256u + threadIdx.x;
    if (word >= words) return;
    uint64_t roots = nodeRoots[word];
    for (uint32_t k = counts[2u * word]; roots && k < K; ++k) {
        nodes[k].first = word * 64u + comp_ctz(roots);
        roots &= roots - 1ull;
    }
    roots = curveRoots[word];
    for (uint32_t b = counts[2u * word + 1u]; roots && b < B; ++b) {
        branches[b].first = word * 64u + comp_ctz(roots);
        roots &= roots - 1ull;
    }
}

__device__ __forceinline__ uint32_t skel_stat_load(const uint32_t* at) { return __hip_atomic_load(at, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void skel_stat_add(uint32_t* at, uint32_t v)
{
    if (v) (void)__hip_atomic_fetch_add(at, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// a minimum, a maximum, flags: sent only where they change what a relaxed agent-scope load shows (the word only moves one way)
__device__ __forceinline__ void skel_stat_min(uint32_t* at, uint32_t v)
{
    if (v < skel_stat_load(at)) (void)__hip_atomic_fetch_min(at, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void skel_stat_max(uint32_t* at, uint32_t v)
{
    if (v > skel_stat_load(at)) (void)__hip_atomic_fetch_max(at, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void skel_stat_or(uint32_t* at, uint32_t v)
{
    if (v & ~skel_stat_load(at)) (void)__hip_atomic_fetch_or(at, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// one lane per mask word: its runs of node voxels, then its runs of curve voxels.  A run has one label: its voxels are adjacent along x and of
// one kind.  The loop over the node runs is the wave's (lanes without a run left take part with len = 0), so that the wave's lanes can be asked
// whether they all hold one label: then the wave reduces its runs in registers and one lane sends the total (components.hip: k_comp_stats) --
// a solid blob is one node, and its record would otherwise take an atomic per run.
__global__ __launch_bounds__(256) void k_skel_stats(const uint64_t* __restrict__ member, const uint64_t* __restrict__ node, const uint64_t* __restrict__ curve,
                                                    const uint64_t* __restrict__ ends, uint32_t N, const uint32_t* __restrict__ labels, const uint32_t* __restrict__ weights,
                                                    SkelNodeStats* stats, uint32_t K, SkelBranch* branches, uint32_t B, uint32_t words)
{
    const uint32_t t = blockIdx.x * 256u + threadIdx.x, lane = threadIdx.x & 63u;
    const bool live = t < words && member[t] != 0ull;
    if (!__any(live)) return;                                           // (the whole wave)
    const uint32_t W = fill_row_words(N), row = live ? t / W : 0u, w = live ? t - row * W : 0u;
    const uint32_t y = row % N, z = row / N, base = row * N + 64u * w;
    const uint64_t e = live ? ends[t] : 0ull;
    uint64_t m = live ? node[t] : 0ull;
    while (__any(m != 0ull)) {
        uint32_t label = 0, len = 0, s = 0;
        if (m) {
            comp_take_run(m, s, len);
            label = labels[base + s];
            if (label == 0u || label > K) len = 0u;                     // (never: a node voxel has a label 1 .. K; no index leaves the table)
        }
        const uint64_t act = __ballot(len != 0u);
        if (!act) continue;
        const uint32_t lead = comp_ctz(act);
        const uint32_t firstLabel = (uint32_t)__shfl((int)label, (int)lead);
        // what this lane's run adds to its node: voxels, the box (x0 .. x1, y, z), the flags, the greatest weight; nothing for a lane without a run
        const uint32_t x0 = 64u * w + s, x1 = x0 + (len ? len - 1u : 0u);
        const uint64_t run = len ? (len == 64u ? ~0ull : (1ull << len) - 1ull) << s : 0ull;
        uint32_t add = len, wMax = 0u;
        uint32_t flags = len ? (comp_run_flags(N, x0, x1, y, z) ? SKEL_NODE_BORDER : 0u) | ((run & e) ? SKEL_NODE_END : 0u) | ((run & ~e) ? SKEL_NODE_JUNCTION : 0u) : 0u;
        uint32_t lo0 = len ? x0 : 0xffffffffu, lo1 = len ? y : 0xffffffffu, lo2 = len ? z : 0xffffffffu;
        uint32_t hi0 = len ? x1 : 0u, hi1 = len ? y : 0u, hi2 = len ? z : 0u;
        if (weights)
            for (uint32_t k = 0; k < len; ++k) wMax = max(wMax, weights[base + s + k]);
        bool sends = len != 0u;
        if (__ballot(len != 0u && label != firstLabel) == 0ull) {       // one label in the whole wave: one lane sends the wave's total
#pragma unroll
            for (uint32_t d = 1; d < 64u; d <<= 1) {
                add += (uint32_t)__shfl_xor((int)add, (int)d);
                flags |= (uint32_t)__shfl_xor((int)flags, (int)d);
                wMax = max(wMax, (uint32_t)__shfl_xor((int)wMax, (int)d));
                lo0 = min(lo0, (uint32_t)__shfl_xor((int)lo0, (int)d)); lo1 = min(lo1, (uint32_t)__shfl_xor((int)lo1, (int)d)); lo2 = min(lo2, (uint32_t)__shfl_xor((int)lo2, (int)d));
                hi0 = max(hi0, (uint32_t)__shfl_xor((int)hi0, (int)d)); hi1 = max(hi1, (uint32_t)__shfl_xor((int)hi1, (int)d)); hi2 = max(hi2, (uint32_t)__shfl_xor((int)hi2, (int)d));
            }
            sends = lane == lead;
        }
        if (sends) {
            SkelNodeStats* st = stats + (label - 1u);
            skel_stat_add(&st->voxels, add);
            skel_stat_min(&st->lo[0], lo0); skel_stat_min(&st->lo[1], lo1); skel_stat_min(&st->lo[2], lo2);
            skel_stat_max(&st->hi[0], hi0); skel_stat_max(&st->hi[1], hi1); skel_stat_max(&st->hi[2], hi2);
            skel_stat_or(&st->flags, flags);
            if (weights) skel_stat_max(&st->w_max, wMax);
        }
    }
    if (!live) return;
    m = curve[t];
    while (m) {
        uint32_t s, len;
        comp_take_run(m, s, len);
        const uint32_t label = labels[base + s], b = label & ~kSkelBranchBit;
        if (!(label & kSkelBranchBit) || b == 0u || b > B) continue;    // (never: a curve voxel has a branch's label 1 .. B)
        SkelBranch* br = branches + (b - 1u);
        const uint32_t x0 = 64u * w + s, x1 = x0 + len - 1u;
        uint32_t steps[3] = {0u, 0u, 0u}, wMin = 0xffffffffu, wMax = 0u;
        unsigned long long wSum = 0ull;
        for (uint32_t k = 0; k < len; ++k) {
            const uint32_t p = base + s + k;
            if (weights) {
                const uint32_t v = weights[p];
                wMin = min(wMin, v); wMax = max(wMax, v); wSum += v;
            }
            skel_neighbours(member, curve, N, y, z, w, s + k, [&](uint32_t q, int dx, int dy, int dz, bool isCurve) {
                const uint32_t type = skel_step_type(dx, dy, dz);
                if (isCurve) {
                    if (p < q) { if (type == 0u) ++steps[0]; else if (type == 1u) ++steps[1]; else ++steps[2]; }
                    return;
                }
                if (type == 0u) ++steps[0]; else if (type == 1u) ++steps[1]; else ++steps[2];
                const uint32_t k2 = labels[q];
                if (k2 == 0u || k2 > K) return;                         // (never: a node voxel)
                skel_stat_min(&br->a, k2);
                skel_stat_max(&br->b, k2);
                skel_stat_add(&stats[k2 - 1u].degree, 1u);
            });
        }
        skel_stat_add(&br->voxels, len);
        skel_stat_add(&br->steps[0], steps[0]); skel_stat_add(&br->steps[1], steps[1]); skel_stat_add(&br->steps[2], steps[2]);
        if (comp_run_flags(N, x0, x1, y, z)) skel_stat_or(&br->flags, SKEL_BRANCH_BORDER);
        if (weights) {
            skel_stat_min(&br->w_min, wMin);
            skel_stat_max(&br->w_max, wMax);
            if (wSum) (void)__hip_atomic_fetch_add(reinterpret_cast<unsigned long long*>(&br->w_sum), wSum, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

__global__ __launch_bounds__(256) void k_skel_nodes(const SkelNodeStats* __restrict__ stats, SkelNode* nodes, uint32_t K)
{
    const uint32_t k = blockIdx.x * 256u + threadIdx.x;
    if (k >= K) return;
    nodes[k] = skel_node_record(nodes[k].first, stats[k]);
}
__global__ __launch_bounds__(256) void k_skel_branches(const SkelNode* __restrict__ nodes, uint32_t K, SkelBranch* branches, uint32_t B, uint32_t weights)
{
    const uint32_t b = blockIdx.x * 256u + threadIdx.x;
    if (b >= B) return;
    SkelBranch r = branches[b];
    if (r.a != kCompNone && (r.a == 0u || r.a > K || r.b == 0u || r.b > K)) return;      // (never: an attachment names a node 1 .. K)
    skel_finish_branch(r, nodes, weights != 0u);
    branches[b] = r;
}

// counters: {branches removed, voxels removed}; goB, goN: a byte per branch and per node, cleared in front of this kernel
__global__ __launch_bounds__(256) void k_skel_prune_mark(const SkelNode* __restrict__ nodes, uint32_t K, const SkelBranch* __restrict__ branches, uint32_t B, uint32_t maxLen345,
                                                         uint8_t* __restrict__ goB, uint8_t* __restrict__ goN, unsigned long long* counters)
{
    const uint32_t b = blockIdx.x * 256u + threadIdx.x;
    if (b >= B) return;
    const SkelBranch r = branches[b];
    if (!skel_pruned(r, maxLen345) || r.a == 0u || r.a > K || r.b == 0u || r.b > K) return;
    goB[b] = 1u;
    goN[skel_spur_tip(r, nodes) - 1u] = 1u;
    (void)__hip_atomic_fetch_add(counters + 0, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    (void)__hip_atomic_fetch_add(counters + 1, (unsigned long long)r.voxels + 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// eight consecutive voxels per thread: two 16-byte loads of labels, one 8-byte load of the grid, a store only where a byte changed
__global__ __launch_bounds__(256) void k_skel_prune_edit(uint8_t* grid, const uint32_t* __restrict__ labels, uint32_t groups, uint32_t K, uint32_t B,
                                                         const uint8_t* __restrict__ goB, const uint8_t* __restrict__ goN)
{
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    if (t >= groups) return;
    const uint4 a = reinterpret_cast<const uint4*>(labels)[2u * (size_t)t], b = reinterpret_cast<const uint4*>(labels)[2u * (size_t)t + 1u];
    const uint32_t l[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
    if (!(a.x | a.y | a.z | a.w | b.x | b.y | b.z | b.w)) return;
    uint64_t* at = reinterpret_cast<uint64_t*>(grid) + t;
    const uint64_t before = *at;
    uint64_t after = before;
#pragma unroll
    for (uint32_t k = 0; k < 8u; ++k) {
        const uint32_t number = l[k] & ~kSkelBranchBit;
        if (number == 0u) continue;
        const bool goes = (l[k] & kSkelBranchBit) ? (number <= B && goB[number - 1u] != 0u) : (number <= K && goN[number - 1u] != 0u);
        if (goes) after &= ~(0xffull << 8u * k);
    }
    if (after != before) *at = after;
}

static uint32_t skel_total(uint32_t N) { return N * N * N; }
static uint32_t skel_linear_words(uint32_t N) { return (skel_total(N) + 63u) / 64u; }

// scratch of one build: the member, node, curve and end masks (a bit per voxel each), the two kinds' root bits in linear order, a pair of counts
// per 64 voxels, the scan's block sums, {K, B, end voxels, curve voxels, junction voxels}
size_t skel_scratch_bytes(uint32_t N)
{
    const size_t words = skel_linear_words(N), mask = align256(fill_mask_words(N) * sizeof(uint64_t));
    return 4u * mask + 2u * align256(words * sizeof(uint64_t)) + align256(words * 2u * sizeof(uint32_t)) + align256((size_t)scan_blocks(words) * 2u * sizeof(unsigned long long)) +
           align256(5u * sizeof(unsigned long long));
}
void skel_scratch_layout(uint8_t* scratch, uint32_t N, SkelParams& p)
{
    const size_t words = skel_linear_words(N), mask = align256(fill_mask_words(N) * sizeof(uint64_t));
    p.N = N;
    p.member = reinterpret_cast<uint64_t*>(scratch);
    p.node = reinterpret_cast<uint64_t*>(scratch + mask);
    p.curve = reinterpret_cast<uint64_t*>(scratch + 2u * mask);
    p.ends = reinterpret_cast<uint64_t*>(scratch + 3u * mask);
    scratch += 4u * mask;
    p.nodeRoots = reinterpret_cast<uint64_t*>(scratch);
    scratch += align256(words * sizeof(uint64_t));
    p.curveRoots = reinterpret_cast<uint64_t*>(scratch);
    scratch += align256(words * sizeof(uint64_t));
    p.counts = reinterpret_cast<uint32_t*>(scratch);
    scratch += align256(words * 2u * sizeof(uint32_t));
    p.sums = reinterpret_cast<unsigned long long*>(scratch);
    scratch += align256((size_t)scan_blocks(words) * 2u * sizeof(unsigned long long));
    p.totals = reinterpret_cast<unsigned long long*>(scratch);
}

static bool skel_params_ok(const SkelParams& p)
{
    return skel_valid(p.N) && p.grid && p.labels && p.member && p.node && p.curve && p.ends && p.nodeRoots && p.curveRoots && p.counts && p.sums && p.totals;
}

// the classify pass alone, over a packed member mask (dxv_skeleton_async; the measurement of the pass by itself)
hipError_t launch_skel_classify(const SkelParams& p, hipStream_t s)
{
    if (!skel_params_ok(p)) return hipErrorInvalidValue;
    const uint32_t N = p.N, maskWords = N * N * fill_row_words(N);
    const size_t mask = align256(fill_mask_words(N) * sizeof(uint64_t));
    hipError_t e = hipMemsetAsync(p.node, 0, 3u * mask, s);            // node, curve and ends stand one behind the other
    if (e != hipSuccess) return e;
    e = hipMemsetAsync(p.totals, 0, 5u * sizeof(unsigned long long), s);
    if (e != hipSuccess) return e;
    k_skel_classify<<<(maskWords + 255u) / 256u, 256, 0, s>>>(p.member, N, p.node, p.curve, p.ends, p.totals + 2, maskWords);
    return hipGetLastError();
}

// pack .. number: p.labels holds the labels, p.totals = {K, B, end voxels, curve voxels, junction voxels}
hipError_t launch_skel_label(const SkelParams& p, hipStream_t s)
{
    if (!skel_params_ok(p)) return hipErrorInvalidValue;
    const uint32_t N = p.N, total = skel_total(N), words = skel_linear_words(N);
    hipError_t e = launch_comp_pack(p.grid, N, COMP_SOLID, p.member, s);
    if (e != hipSuccess) return e;
    e = launch_skel_classify(p, s);
    if (e != hipSuccess) return e;
    k_skel_init<<<(total / 4u + 255u) / 256u, 256, 0, s>>>(p.node, p.curve, N, p.labels, total);
    e = launch_comp_merge(p.node, N, 26u, p.labels, s);
    if (e != hipSuccess) return e;
    e = launch_comp_merge(p.curve, N, 26u, p.labels, s);
    if (e != hipSuccess) return e;
    e = launch_comp_compress(p.labels, N, s);
    if (e != hipSuccess) return e;
    k_skel_roots<<<(words + 3u) / 4u, 256, 0, s>>>(p.labels, p.curve, N, total, p.nodeRoots, p.curveRoots, p.counts, words);
    e = launch_scan_words(p.counts, 2, words, p.sums, p.totals, s);
    if (e != hipSuccess) return e;
    k_skel_number<<<(total / 4u + 255u) / 256u, 256, 0, s>>>(p.labels, total, p.nodeRoots, p.curveRoots, p.counts);
    return hipGetLastError();
}

// the tables of the K nodes and B branches launch_skel_label found (K + B >= 1); p.stats: K SkelNodeStats of scratch
hipError_t launch_skel_stats(const SkelParams& p, uint32_t K, uint32_t B, hipStream_t s)
{
    if (!skel_params_ok(p) || !(K | B) || (K && (!p.stats || !p.nodes)) || (B && !p.branches)) return hipErrorInvalidValue;
    const uint32_t N = p.N, maskWords = N * N * fill_row_words(N), words = skel_linear_words(N), most = K > B ? K : B;
    k_skel_stats_init<<<(most + 255u) / 256u, 256, 0, s>>>(p.stats, K, p.branches, B);
    k_skel_first<<<(words + 255u) / 256u, 256, 0, s>>>(p.nodeRoots, p.curveRoots, p.counts, words, p.nodes, K, p.branches, B);
    k_skel_stats<<<(maskWords + 255u) / 256u, 256, 0, s>>>(p.member, p.node, p.curve, p.ends, N, p.labels, p.weights, p.stats, K, p.branches, B, maskWords);
    if (K) k_skel_nodes<<<(K + 255u) / 256u, 256, 0, s>>>(p.stats, p.nodes, K);
    if (B) k_skel_branches<<<(B + 255u) / 256u, 256, 0, s>>>(p.nodes, K, p.branches, B, p.weights ? 1u : 0u);
    return hipGetLastError();
}

size_t skel_prune_bytes(uint32_t K, uint32_t B) { return align256(2u * sizeof(unsigned long long)) + align256(B) + align256(K); }
unsigned long long* skel_prune_counters(uint8_t* work) { return reinterpret_cast<unsigned long long*>(work); }

// the grid edited from its skeleton: `work` holds the two counters, then B flags and K flags
hipError_t launch_skel_prune(uint8_t* grid, uint32_t N, const uint32_t* labels, const SkelNode* nodes, uint32_t K, const SkelBranch* branches, uint32_t B, uint32_t maxLen345,
                             uint8_t* work, hipStream_t s)
{
    if (!skel_valid(N) || !grid || !labels || !work || (K && !nodes) || (B && !branches)) return hipErrorInvalidValue;
    const hipError_t e = hipMemsetAsync(work, 0, skel_prune_bytes(K, B), s);
    if (e != hipSuccess) return e;
    if (!B || !K) return hipSuccess;                                    // (a spur has a tip)
    uint8_t* goB = work + align256(2u * sizeof(unsigned long long));
    uint8_t* goN = goB + align256(B);
    const uint32_t groups = skel_total(N) / 8u;
    k_skel_prune_mark<<<(B + 255u) / 256u, 256, 0, s>>>(nodes, K, branches, B, maxLen345, goB, goN, skel_prune_counters(work));
    k_skel_prune_edit<<<(groups + 255u) / 256u, 256, 0, s>>>(grid, labels, groups, K, B, goB, goN);
    return hipGetLastError();
}

} // namespace dxv
