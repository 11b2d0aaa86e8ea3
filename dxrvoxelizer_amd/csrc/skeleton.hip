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
//   k_label_roots<2>   dxv_label.h, the components' numbering for two kinds of root: a wave per 64 voxels in linear order, the node roots and
//                      the curve roots -- the roots whose voxel is in the curve mask -- as bits, and their two counts
//   scan.hip           the exclusive scan of the count pairs (launch_scan_words, C = 2); the totals {K, B} are what the host reads
//   k_label_number<2>  labels[p] = rank of p's root among its kind's roots + 1, with bit 31 for a branch; in place
//   k_skel_stats_init, k_label_first<2>, k_skel_stats, k_skel_nodes, k_skel_branches
//                      behind the host's read of K and B: `first` from the root bits into the two tables; one lane per mask word gathers a set of
//                      sums, minima, maxima and ORs per run of node voxels (BoxRun, dxv_label.h, with the greatest weight beside it) and per run
//                      of curve voxels (one label each) and sends it with integer atomics; the steps and attachments of every curve voxel from
//                      its neighbours (skel_neighbours); then the records, nodes before branches
//   k_skel_prune_mark, k_label_edit<SkelGoes>
//                      dxv_skeleton_prune: a flag per branch and per tip from the tables, two counters; one pass over labels and grid
//                      (dxv_label.h) with the flags as its predicate
// Every loop is bounded by the bits of a word or by the 26 neighbours; no kernel here uses scratch memory or LDS, none waits for another workgroup.
// The scratch is described once, by skel_carve and skel_prune_carve (dxv_skeleton.h).
#include "dxv_device.h"
#include "dxv_skeleton.h"
#include "dxv_label.h"

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

__global__ __launch_bounds__(256) void k_skel_stats_init(SkelNodeStats* __restrict__ stats, uint32_t K, SkelBranch* __restrict__ branches, uint32_t B)
{
    const uint32_t k = blockIdx.x * 256u + threadIdx.x;
    if (k < K) {
        SkelNodeStats s;
        static_cast<BoxStats&>(s) = box_stats_none();
        s.degree = 0u; s.w_max = 0u;
        stats[k] = s;
    }
    if (k < B) {
        SkelBranch r;
        r.a = kCompNone; r.b = 0u; r.first = 0u; r.voxels = 0u; r.steps[0] = r.steps[1] = r.steps[2] = 0u; r.flags = 0u;
        r.w_min = 0xffffffffu; r.w_max = 0u; r.w_sum = 0ull;
        branches[k] = r;
    }
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
        const uint64_t bits = len ? (len == 64u ? ~0ull : (1ull << len) - 1ull) << s : 0ull;
        BoxRun run(len != 0u, len, x0, x1, y, z, (comp_run_flags(N, x0, x1, y, z) ? SKEL_NODE_BORDER : 0u) | ((bits & e) ? SKEL_NODE_END : 0u) | ((bits & ~e) ? SKEL_NODE_JUNCTION : 0u));
        uint32_t wMax = 0u;
        if (weights)
            for (uint32_t k = 0; k < len; ++k) wMax = max(wMax, weights[base + s + k]);
        bool sends = len != 0u;
        if (__ballot(len != 0u && label != firstLabel) == 0ull) {       // one label in the whole wave: one lane sends the wave's total
            run.reduce_wave();
#pragma unroll
            for (uint32_t d = 1; d < 64u; d <<= 1) wMax = max(wMax, (uint32_t)__shfl_xor((int)wMax, (int)d));
            sends = lane == lead;
        }
        if (sends) {
            SkelNodeStats* st = stats + (label - 1u);
            run.send(st);
            if (weights) stat_max(&st->w_max, wMax);
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
                stat_min(&br->a, k2);
                stat_max(&br->b, k2);
                stat_add(&stats[k2 - 1u].degree, 1u);
            });
        }
        stat_add(&br->voxels, len);
        stat_add(&br->steps[0], steps[0]); stat_add(&br->steps[1], steps[1]); stat_add(&br->steps[2], steps[2]);
        if (comp_run_flags(N, x0, x1, y, z)) stat_or(&br->flags, SKEL_BRANCH_BORDER);
        if (weights) {
            stat_min(&br->w_min, wMin);
            stat_max(&br->w_max, wMax);
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

// which labels leave under a prune, for k_label_edit: the branches and the tips k_skel_prune_mark flagged
struct SkelGoes {
    uint32_t K, B;
    const uint8_t *goB, *goN;
    __device__ __forceinline__ bool becomes() const { return false; }
    __device__ __forceinline__ uint32_t prepare() const { return 0u; }
    __device__ __forceinline__ bool operator()(uint32_t label, uint32_t) const
    {
        const uint32_t number = label & ~kSkelBranchBit;
        if (number == 0u) return false;
        return (label & kSkelBranchBit) ? (number <= B && goB[number - 1u] != 0u) : (number <= K && goN[number - 1u] != 0u);
    }
};

static uint32_t skel_total(uint32_t N) { return N * N * N; }

static bool skel_params_ok(const SkelParams& p)
{
    return skel_valid(p.N) && p.grid && p.labels && p.member && p.node && p.curve && p.ends && p.nodeRoots && p.curveRoots && p.counts && p.sums && p.totals;
}

// the classify pass alone, over a packed member mask (dxv_skeleton_async; the measurement of the pass by itself)
hipError_t launch_skel_classify(const SkelParams& p, hipStream_t s)
{
    if (!skel_params_ok(p)) return hipErrorInvalidValue;
    const uint32_t N = p.N, maskWords = N * N * fill_row_words(N);
    hipError_t e = hipMemsetAsync(p.node, 0, 3u * fill_mask_bytes(N), s);      // node, curve and ends stand one behind the other (skel_carve)
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
    const uint32_t N = p.N, total = skel_total(N), words = comp_linear_words(N);
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
    k_label_roots<2><<<(words + 3u) / 4u, 256, 0, s>>>(p.labels, p.curve, N, total, p.nodeRoots, p.curveRoots, p.counts, words);
    e = launch_scan_words(p.counts, 2, words, p.sums, p.totals, s);
    if (e != hipSuccess) return e;
    k_label_number<2><<<(total / 4u + 255u) / 256u, 256, 0, s>>>(p.labels, total, p.nodeRoots, p.curveRoots, p.counts);
    return hipGetLastError();
}

// the tables of the K nodes and B branches launch_skel_label found (K + B >= 1); p.stats: K SkelNodeStats of scratch
hipError_t launch_skel_stats(const SkelParams& p, uint32_t K, uint32_t B, hipStream_t s)
{
    if (!skel_params_ok(p) || !(K | B) || (K && (!p.stats || !p.nodes)) || (B && !p.branches)) return hipErrorInvalidValue;
    const uint32_t N = p.N, maskWords = N * N * fill_row_words(N), words = comp_linear_words(N), most = K > B ? K : B;
    k_skel_stats_init<<<(most + 255u) / 256u, 256, 0, s>>>(p.stats, K, p.branches, B);
    k_label_first<2, SkelNode, SkelBranch><<<(words + 255u) / 256u, 256, 0, s>>>(p.nodeRoots, p.curveRoots, p.counts, words, p.nodes, K, p.branches, B);
    k_skel_stats<<<(maskWords + 255u) / 256u, 256, 0, s>>>(p.member, p.node, p.curve, p.ends, N, p.labels, p.weights, p.stats, K, p.branches, B, maskWords);
    if (K) k_skel_nodes<<<(K + 255u) / 256u, 256, 0, s>>>(p.stats, p.nodes, K);
    if (B) k_skel_branches<<<(B + 255u) / 256u, 256, 0, s>>>(p.nodes, K, p.branches, B, p.weights ? 1u : 0u);
    return hipGetLastError();
}

// the grid edited from its skeleton: `work` (skel_prune_carve) holds the two counters, then B flags and K flags
hipError_t launch_skel_prune(uint8_t* grid, uint32_t N, const uint32_t* labels, const SkelNode* nodes, uint32_t K, const SkelBranch* branches, uint32_t B, uint32_t maxLen345,
                             const SkelPruneWork& work, hipStream_t s)
{
    if (!skel_valid(N) || !grid || !labels || !work.counters || !work.goB || !work.goN || (K && !nodes) || (B && !branches)) return hipErrorInvalidValue;
    const hipError_t e = hipMemsetAsync(work.counters, 0, work.bytes, s);
    if (e != hipSuccess) return e;
    if (!B || !K) return hipSuccess;                                    // (a spur has a tip)
    const uint32_t groups = skel_total(N) / 8u;
    k_skel_prune_mark<<<(B + 255u) / 256u, 256, 0, s>>>(nodes, K, branches, B, maxLen345, work.goB, work.goN, work.counters);
    k_label_edit<<<(groups + 255u) / 256u, 256, 0, s>>>(grid, labels, groups, SkelGoes{K, B, work.goB, work.goN});
    return hipGetLastError();
}

} // namespace dxv
