// components.hip -- the connected components of a whole N^3 grid (dxv_components.h has the rule's word routines and the union-find), on the
// frame's stream.  One pass over the mask, no fixed-point rounds, nothing for the host to settle:
//   k_comp_pack        grid (1 B per voxel) -> the member mask (1 bit per voxel, the fill's layout; inverted for DXV_COMP_EMPTY): the one read
//                      of the grid
//   k_comp_init        parent[p] = the start of p's run inside its own mask word, kCompNone for a non-member.  parent IS the label buffer.
//   k_comp_merge       one lane per mask word: the link to the word before it in the row and the unions with the earlier neighbour rows
//                      (comp_merge_word).  EVERY access to parent in this kernel is an agent-scope relaxed atomic -- loads, and
//                      fetch_min for every write (CompAtomic) --, vector instructions that are served by the L2 all CUs share: no decision
//                      rests on a CU's L1 copy.  And no decision needs a FRESH value either: parent[i] only ever falls and only ever points
//                      into i's own component, and a hook that finds its root already hooked (old != a) goes on from what it found.  That
//                      hook may have moved a under b before old's set and b's are joined: the trees are right when the kernel ENDS, not
//                      at every instant inside it (dxv_components.h, head comment), and nothing reads them before.
//   k_comp_compress    behind the kernel boundary: parent[p] = the root of p = first(C).  Plain accesses: other lanes write roots into
//                      entries this lane reads, and whichever of the two values it sees is an ancestor of p.
//   k_label_roots<1>   dxv_label.h: one bit per voxel in linear order, parent[p] == p, and their count per 64 voxels
//   scan.hip           the exclusive scan of those counts (launch_scan_words, one count per word); the total, K, is what the host reads
//   k_label_number<1>  dxv_label.h: labels[p] = rank(root) + 1, in place (a lane reads only its own entry of the buffer it writes)
//   k_comp_stats_init, k_label_first<1>, k_comp_stats, k_comp_table
//                      behind the host's read of K: `first` from the root bits; voxels, lo, hi and flags by integer atomics into 32-bit words
//                      -- sums, minima, maxima and an OR: no arrival order shows --, one lane per mask word and one load of a label per RUN;
//                      when every run a wave holds in a step has one label, the wave reduces its runs in registers and one lane sends the
//                      total, and a minimum, maximum or flag that would change nothing is not sent (BoxRun, dxv_label.h); then the 24-byte
//                      records.
//   k_comp_keep, k_label_edit<CompGoes>
//                      dxv_components_select: one kernel over the table (keep flags, the 64-bit maximum of voxels << 32 | ~number, three
//                      counters), one pass over labels and grid (dxv_label.h) with the rule's predicate.
// launch_comp_merge and launch_comp_compress run k_comp_merge and k_comp_compress alone, for skeleton.hip, which labels two disjoint masks over one
// parent array and numbers their roots with the same kernels at C = 2.  The scratch is described once, by comp_carve (dxv_components.h).
// Every loop ends because an index strictly falls (comp_find, comp_root, comp_union) or bits leave a word (the run loops).  No loop waits for
// another workgroup, no kernel here uses scratch memory or LDS.
#include "dxv_device.h"
#include "dxv_components.h"
#include "dxv_label.h"

namespace dxv {

// parent[] as the merge kernel sees it
struct CompAtomic {
    uint32_t* p;
    __device__ __forceinline__ uint32_t load(uint32_t i) const { return __hip_atomic_load(p + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
    __device__ __forceinline__ uint32_t lower(uint32_t i, uint32_t v) const { return __hip_atomic_fetch_min(p + i, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
};
// ... and the compress kernel
struct CompPlain {
    const uint32_t* p;
    __device__ __forceinline__ uint32_t load(uint32_t i) const { return p[i]; }
};

// one thread per byte of a mask row (W * 8 of them, the ones behind the row's end are 0)
__global__ __launch_bounds__(256) void k_comp_pack(const uint8_t* __restrict__ grid, uint32_t N, int of, uint8_t* __restrict__ mask)
{
    const uint32_t rowBytes = fill_row_words(N) * 8u;
    const size_t t = (size_t)blockIdx.x * 256u + threadIdx.x;
    if (t >= (size_t)N * N * rowBytes) return;
    const size_t row = t / rowBytes;
    const uint32_t j = (uint32_t)(t % rowBytes);
    uint32_t bits = 0;
    if (8u * j < N) {
        const uint8_t* g = grid + row * N;
        bits = (N & 7u) ? comp_member_byte(g, N, j, of) : comp_member_byte(*reinterpret_cast<const uint64_t*>(g + 8u * j), of);
    }
    mask[t] = (uint8_t)bits;
}

// four consecutive voxels per thread (N is even: N^3 is a multiple of 8)
__global__ __launch_bounds__(256) void k_comp_init(const uint64_t* __restrict__ mask, uint32_t N, uint32_t* __restrict__ parent, uint32_t total)
{
    const size_t first = ((size_t)blockIdx.x * 256u + threadIdx.x) * 4u;
    if (first >= total) return;
    const uint32_t p = (uint32_t)first;
    *reinterpret_cast<uint4*>(parent + p) = make_uint4(comp_init_parent(mask, N, p), comp_init_parent(mask, N, p + 1u), comp_init_parent(mask, N, p + 2u),
                                                       comp_init_parent(mask, N, p + 3u));
}

__global__ __launch_bounds__(256) void k_comp_merge(const uint64_t* __restrict__ mask, uint32_t N, uint32_t connectivity, uint32_t* parent, uint32_t words)
{
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    if (t >= words) return;
    const uint32_t W = fill_row_words(N), row = t / W;
    CompAtomic par{parent};
    comp_merge_word(par, mask, N, connectivity, row % N, row / N, t - row * W);
}

__global__ __launch_bounds__(256) void k_comp_compress(uint32_t* parent, uint32_t total)
{
    const size_t i = (size_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= total) return;
    const uint32_t p = (uint32_t)i, pa = parent[p];
    if (pa == kCompNone || pa == p) return;
    CompPlain par{parent};
    const uint32_t root = comp_root(par, pa);
    if (root != pa) parent[p] = root;
}

__global__ __launch_bounds__(256) void k_comp_stats_init(CompStats* __restrict__ stats, uint32_t K)
{
    const uint32_t k = blockIdx.x * 256u + threadIdx.x;
    if (k < K) stats[k] = box_stats_none();
}

// one lane per mask word, a step of the loop per run of the lane's word; the loop is the wave's (lanes without a run left take part with
// len = 0), so that the wave's lanes can be asked whether they all hold one label
__global__ __launch_bounds__(256) void k_comp_stats(const uint64_t* __restrict__ mask, uint32_t N, const uint32_t* __restrict__ labels, CompStats* stats, uint32_t words,
                                                    uint32_t K)
{
    const uint32_t t = blockIdx.x * 256u + threadIdx.x, lane = threadIdx.x & 63u;
    const uint32_t W = fill_row_words(N);
    uint64_t m = 0;
    uint32_t row = 0, w = 0;
    if (t < words) { row = t / W; w = t - row * W; m = mask[t]; }
    const uint32_t y = row % N, z = row / N, base = row * N + 64u * w;
    while (__any(m != 0ull)) {
        uint32_t label = 0, len = 0, s = 0;
        if (m) {
            comp_take_run(m, s, len);
            label = labels[base + s];
            if (label == 0u || label > K) len = 0u;                     // (never: a member has a label 1 .. K; no index leaves the table)
        }
        const uint64_t act = __ballot(len != 0u);
        if (!act) continue;
        const uint32_t lead = comp_ctz(act);
        const uint32_t firstLabel = (uint32_t)__shfl((int)label, (int)lead);
        // what this lane's run adds to its component: voxels, the box (x0 .. x1, y, z) and the border flag; nothing for a lane without a run
        const uint32_t x0 = 64u * w + s, x1 = x0 + (len ? len - 1u : 0u);
        BoxRun run(len != 0u, len, x0, x1, y, z, comp_run_flags(N, x0, x1, y, z));
        bool sends = len != 0u;
        if (__ballot(len != 0u && label != firstLabel) == 0ull) {       // one label in the whole wave: one lane sends the wave's total
            run.reduce_wave();
            sends = lane == lead;
        }
        if (sends) run.send(stats + (label - 1u));
    }
}

__global__ __launch_bounds__(256) void k_comp_table(const CompStats* __restrict__ stats, CompRecord* table, uint32_t K)
{
    const uint32_t k = blockIdx.x * 256u + threadIdx.x;
    if (k >= K) return;
    table[k] = comp_record(table[k].first, stats[k]);
}

// counters: {kept, dropped, voxels changed, the maximum of comp_best_key}.  DXV_SELECT_LARGEST: who is kept is known only once the maximum is,
// so this kernel counts every component as dropped and every voxel as changed, and whoever reads the four words takes the one kept
// component out again (comp_select_counts); the edit pass compares a label with the maximum instead of reading a flag.
__global__ __launch_bounds__(256) void k_comp_keep(const CompRecord* __restrict__ table, uint32_t K, int rule, uint32_t arg, uint8_t* __restrict__ keep,
                                                   unsigned long long* counters)
{
    const uint32_t k = blockIdx.x * 256u + threadIdx.x, lane = threadIdx.x & 63u;
    unsigned long long kept = 0, dropped = 0, changed = 0, best = 0;
    if (k < K) {
        const uint32_t voxels = table[k].voxels;
        const bool keeps = rule != COMP_SELECT_LARGEST && comp_keep(rule, arg, k + 1u, voxels, table[k].flags, 0ull);
        keep[k] = keeps ? 1u : 0u;
        kept = keeps ? 1u : 0u; dropped = keeps ? 0u : 1u; changed = keeps ? 0u : voxels;
        best = comp_best_key(voxels, k + 1u);
    }
#pragma unroll
    for (uint32_t d = 1; d < 64u; d <<= 1) {                            // (every lane of the wave is here)
        kept += __shfl_xor(kept, (int)d);
        dropped += __shfl_xor(dropped, (int)d);
        changed += __shfl_xor(changed, (int)d);
        const unsigned long long other = __shfl_xor(best, (int)d);
        best = other > best ? other : best;
    }
    if (lane == 0u && (kept | dropped)) {
        if (kept) (void)__hip_atomic_fetch_add(counters + 0, kept, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (dropped) (void)__hip_atomic_fetch_add(counters + 1, dropped, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (changed) (void)__hip_atomic_fetch_add(counters + 2, changed, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (rule == COMP_SELECT_LARGEST) (void)__hip_atomic_fetch_max(counters + 3, best, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// which labels leave under a select rule, for k_label_edit: DXV_SELECT_LARGEST compares with the maximum k_comp_keep left, the others read its flags
struct CompGoes {
    int of, rule;
    uint32_t K;
    const uint8_t* keep;
    const unsigned long long* counters;
    __device__ __forceinline__ bool becomes() const { return of == COMP_EMPTY; }
    __device__ __forceinline__ uint32_t prepare() const { return rule == COMP_SELECT_LARGEST ? comp_best_number(counters[3]) : 0u; }
    __device__ __forceinline__ bool operator()(uint32_t label, uint32_t best) const
    {
        if (label > K) return false;                                    // (never: a member has a label 1 .. K; no index leaves the flags)
        return rule == COMP_SELECT_LARGEST ? label != best : keep[label - 1u] == 0u;
    }
};

static uint32_t comp_total(uint32_t N) { return N * N * N; }

static bool comp_params_ok(const CompParams& p)
{
    return p.N >= 2u && p.N <= kCompMaxN && !(p.N & 1u) && (p.of == COMP_SOLID || p.of == COMP_EMPTY) && (p.connectivity == 6u || p.connectivity == 26u) && p.grid &&
           p.labels && p.mask && p.rootMask && p.bases && p.sums && p.total;
}

// the pack alone: the member mask of a labelling made again from the grid it was made of (dxv_measure, once dxv_trim has released the mask)
hipError_t launch_comp_pack(const uint8_t* grid, uint32_t N, int of, uint64_t* mask, hipStream_t s)
{
    if (N < 2u || N > kCompMaxN || (N & 1u) || (of != COMP_SOLID && of != COMP_EMPTY) || !grid || !mask) return hipErrorInvalidValue;
    const size_t maskBytes = fill_mask_words(N) * 8u;
    k_comp_pack<<<(uint32_t)((maskBytes + 255u) / 256u), 256, 0, s>>>(grid, N, of, reinterpret_cast<uint8_t*>(mask));
    return hipGetLastError();
}

// the merge alone, and the compress alone: the unions of a mask over a parent array the caller has initialised from it (skeleton.hip: two
// disjoint masks over one array), then every entry its root
hipError_t launch_comp_merge(const uint64_t* mask, uint32_t N, uint32_t connectivity, uint32_t* parent, hipStream_t s)
{
    if (N < 2u || N > kCompMaxN || (N & 1u) || (connectivity != 6u && connectivity != 26u) || !mask || !parent) return hipErrorInvalidValue;
    const uint32_t maskWords = N * N * fill_row_words(N);
    k_comp_merge<<<(maskWords + 255u) / 256u, 256, 0, s>>>(mask, N, connectivity, parent, maskWords);
    return hipGetLastError();
}
hipError_t launch_comp_compress(uint32_t* parent, uint32_t N, hipStream_t s)
{
    if (N < 2u || N > kCompMaxN || (N & 1u) || !parent) return hipErrorInvalidValue;
    const uint32_t total = comp_total(N);
    k_comp_compress<<<(uint32_t)(((size_t)total + 255u) / 256u), 256, 0, s>>>(parent, total);
    return hipGetLastError();
}

// pack .. number: p.labels holds the labels, p.rootMask and p.bases the roots, *p.total = K
hipError_t launch_comp_label(const CompParams& p, hipStream_t s)
{
    if (!comp_params_ok(p)) return hipErrorInvalidValue;
    const uint32_t N = p.N, W = fill_row_words(N), total = comp_total(N), maskWords = N * N * W, words = comp_linear_words(N);
    const size_t maskBytes = (size_t)maskWords * 8u;
    k_comp_pack<<<(uint32_t)((maskBytes + 255u) / 256u), 256, 0, s>>>(p.grid, N, p.of, reinterpret_cast<uint8_t*>(p.mask));
    k_comp_init<<<(total / 4u + 255u) / 256u, 256, 0, s>>>(p.mask, N, p.labels, total);
    k_comp_merge<<<(maskWords + 255u) / 256u, 256, 0, s>>>(p.mask, N, p.connectivity, p.labels, maskWords);
    k_comp_compress<<<(uint32_t)(((size_t)total + 255u) / 256u), 256, 0, s>>>(p.labels, total);
    k_label_roots<1><<<(words + 3u) / 4u, 256, 0, s>>>(p.labels, nullptr, N, total, p.rootMask, nullptr, p.bases, words);
    const hipError_t e = launch_scan_words(p.bases, 1, words, p.sums, p.total, s);
    if (e != hipSuccess) return e;
    k_label_number<1><<<(total / 4u + 255u) / 256u, 256, 0, s>>>(p.labels, total, p.rootMask, nullptr, p.bases);
    return hipGetLastError();
}

// the table of the K components launch_comp_label found (K >= 1); p.stats: K CompStats of scratch
hipError_t launch_comp_stats(const CompParams& p, uint32_t K, hipStream_t s)
{
    if (!comp_params_ok(p) || !K || !p.stats || !p.table) return hipErrorInvalidValue;
    const uint32_t N = p.N, maskWords = N * N * fill_row_words(N), words = comp_linear_words(N);
    k_comp_stats_init<<<(K + 255u) / 256u, 256, 0, s>>>(p.stats, K);
    k_label_first<1, CompRecord, CompRecord><<<(words + 255u) / 256u, 256, 0, s>>>(p.rootMask, nullptr, p.bases, words, p.table, K, nullptr, 0u);
    k_comp_stats<<<(maskWords + 255u) / 256u, 256, 0, s>>>(p.mask, N, p.labels, p.stats, maskWords, K);
    k_comp_table<<<(K + 255u) / 256u, 256, 0, s>>>(p.stats, p.table, K);
    return hipGetLastError();
}

// the grid edited from its labels: `work` (comp_select_carve) holds the four counters, then K keep flags
hipError_t launch_comp_select(uint8_t* grid, uint32_t N, int of, const uint32_t* labels, const CompRecord* table, uint32_t K, int rule, uint32_t arg, const CompSelectWork& work,
                              hipStream_t s)
{
    if (N < 2u || N > kCompMaxN || (N & 1u) || !grid || !labels || !work.counters || !work.keep || (K && !table)) return hipErrorInvalidValue;
    unsigned long long* counters = work.counters;
    uint8_t* keep = work.keep;
    const hipError_t e = hipMemsetAsync(counters, 0, 4u * sizeof(unsigned long long), s);
    if (e != hipSuccess) return e;
    if (!K) return hipSuccess;
    const uint32_t groups = comp_total(N) / 8u;
    k_comp_keep<<<(K + 255u) / 256u, 256, 0, s>>>(table, K, rule, arg, keep, counters);
    k_label_edit<<<(groups + 255u) / 256u, 256, 0, s>>>(grid, labels, groups, CompGoes{of, rule, K, keep, counters});
    return hipGetLastError();
}

} // namespace dxv
