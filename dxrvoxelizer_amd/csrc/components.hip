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
//   k_comp_roots       one bit per voxel in linear order, parent[p] == p, and their count per 64 voxels
//   scan.hip           the exclusive scan of those counts (launch_scan_words, one count per word); the total, K, is what the host reads
//   k_comp_number      labels[p] = rank(root) + 1, in place (a lane reads only its own entry of the buffer it writes)
//   k_comp_stats_init, k_comp_first, k_comp_stats, k_comp_table
//                      behind the host's read of K: `first` from the root bits; voxels, lo, hi and flags by integer atomics into 32-bit words
//                      -- sums, minima, maxima and an OR: no arrival order shows --, one lane per mask word and one load of a label per RUN;
//                      when every run a wave holds in a step has one label, the wave reduces its runs in registers and one lane sends the
//                      total, and a minimum, maximum or flag that would change nothing is not sent; then the 24-byte records.
//   k_comp_keep, k_comp_edit
//                      dxv_components_select: one kernel over the table (keep flags, the 64-bit maximum of voxels << 32 | ~number, three
//                      counters), one pass over labels and grid.
// launch_comp_merge and launch_comp_compress run k_comp_merge and k_comp_compress alone, for skeleton.hip, which labels two disjoint masks over one
// parent array.
// Every loop ends because an index strictly falls (comp_find, comp_root, comp_union) or bits leave a word (the run loops).  No loop waits for
// another workgroup, no kernel here uses scratch memory or LDS.
#include "dxv_device.h"
#include "dxv_components.h"

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

// a wave per 64 voxels in linear order
__global__ __launch_bounds__(256) void k_comp_roots(const uint32_t* __restrict__ parent, uint32_t total, uint64_t* __restrict__ rootMask, uint32_t* __restrict__ bases,
                                                    uint32_t words)
{
    const uint32_t word = blockIdx.x * 4u + (threadIdx.x >> 6);
    if (word >= words) return;                                          // (the whole wave)
    const uint32_t lane = threadIdx.x & 63u;
    const size_t p = (size_t)word * 64u + lane;
    const uint64_t roots = __ballot(p < total && parent[p] == (uint32_t)p);
    if (lane == 0u) { rootMask[word] = roots; bases[word] = comp_popc(roots); }
}

__device__ __forceinline__ uint32_t comp_label_of(uint32_t root, const uint64_t* __restrict__ rootMask, const uint32_t* __restrict__ bases)
{
    return root == kCompNone ? 0u : comp_rank(rootMask, bases, root) + 1u;
}
// four consecutive voxels per thread
__global__ __launch_bounds__(256) void k_comp_number(uint32_t* labels, uint32_t total, const uint64_t* __restrict__ rootMask, const uint32_t* __restrict__ bases)
{
    const size_t first = ((size_t)blockIdx.x * 256u + threadIdx.x) * 4u;
    if (first >= total) return;
    uint4* at = reinterpret_cast<uint4*>(labels + first);
    const uint4 r = *at;
    *at = make_uint4(comp_label_of(r.x, rootMask, bases), comp_label_of(r.y, rootMask, bases), comp_label_of(r.z, rootMask, bases), comp_label_of(r.w, rootMask, bases));
}

__global__ __launch_bounds__(256) void k_comp_stats_init(CompStats* __restrict__ stats, uint32_t K)
{
    const uint32_t k = blockIdx.x * 256u + threadIdx.x;
    if (k >= K) return;
    CompStats s;
    s.voxels = 0u; s.flags = 0u;
    for (int a = 0; a < 3; ++a) { s.lo[a] = 0xffffffffu; s.hi[a] = 0u; }
    stats[k] = s;
}

// one lane per 64 voxels in linear order: the roots among them are the `first` of consecutive components
__global__ __launch_bounds__(256) void k_comp_first(const uint64_t* __restrict__ rootMask, const uint32_t* __restrict__ bases, uint32_t words, CompRecord* __restrict__ table,
                                                    uint32_t K)
{
    const uint32_t word = blockIdx.x * 256u + threadIdx.x;
    if (word >= words) return;
    uint64_t roots = rootMask[word];
    for (uint32_t k = bases[word]; roots && k < K; ++k) {
        table[k].first = word * 64u + comp_ctz(roots);
        roots &= roots - 1ull;
    }
}

// a minimum, a maximum, a flag: sent only where it changes what a relaxed agent-scope load shows (the word only moves one way, so a value
// that has been overtaken costs an atomic that changes nothing, never a missing one)
__device__ __forceinline__ uint32_t comp_stat_load(const uint32_t* at) { return __hip_atomic_load(at, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void comp_stat_min(uint32_t* at, uint32_t v)
{
    if (v < comp_stat_load(at)) (void)__hip_atomic_fetch_min(at, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void comp_stat_max(uint32_t* at, uint32_t v)
{
    if (v > comp_stat_load(at)) (void)__hip_atomic_fetch_max(at, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
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
        uint32_t add = len, flags = len ? comp_run_flags(N, x0, x1, y, z) : 0u;
        uint32_t lo0 = len ? x0 : 0xffffffffu, lo1 = len ? y : 0xffffffffu, lo2 = len ? z : 0xffffffffu;
        uint32_t hi0 = len ? x1 : 0u, hi1 = len ? y : 0u, hi2 = len ? z : 0u;
        bool sends = len != 0u;
        if (__ballot(len != 0u && label != firstLabel) == 0ull) {       // one label in the whole wave: one lane sends the wave's total
#pragma unroll
            for (uint32_t d = 1; d < 64u; d <<= 1) {
                add += (uint32_t)__shfl_xor((int)add, (int)d);
                flags |= (uint32_t)__shfl_xor((int)flags, (int)d);
                lo0 = min(lo0, (uint32_t)__shfl_xor((int)lo0, (int)d)); lo1 = min(lo1, (uint32_t)__shfl_xor((int)lo1, (int)d)); lo2 = min(lo2, (uint32_t)__shfl_xor((int)lo2, (int)d));
                hi0 = max(hi0, (uint32_t)__shfl_xor((int)hi0, (int)d)); hi1 = max(hi1, (uint32_t)__shfl_xor((int)hi1, (int)d)); hi2 = max(hi2, (uint32_t)__shfl_xor((int)hi2, (int)d));
            }
            sends = lane == lead;
        }
        if (sends) {
            CompStats* st = stats + (label - 1u);
            (void)__hip_atomic_fetch_add(&st->voxels, add, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            comp_stat_min(&st->lo[0], lo0); comp_stat_min(&st->lo[1], lo1); comp_stat_min(&st->lo[2], lo2);
            comp_stat_max(&st->hi[0], hi0); comp_stat_max(&st->hi[1], hi1); comp_stat_max(&st->hi[2], hi2);
            if (flags && !comp_stat_load(&st->flags))
                (void)__hip_atomic_fetch_or(&st->flags, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
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

// eight consecutive voxels per thread: two 16-byte loads of labels, one 8-byte load of the grid, a store only where a byte changed
__global__ __launch_bounds__(256) void k_comp_edit(uint8_t* grid, const uint32_t* __restrict__ labels, uint32_t groups, int of, int rule, uint32_t K,
                                                   const uint8_t* __restrict__ keep, const unsigned long long* __restrict__ counters)
{
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    if (t >= groups) return;
    const uint4 a = reinterpret_cast<const uint4*>(labels)[2u * (size_t)t], b = reinterpret_cast<const uint4*>(labels)[2u * (size_t)t + 1u];
    const uint32_t l[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
    const uint32_t bestNumber = rule == COMP_SELECT_LARGEST ? comp_best_number(counters[3]) : 0u;
    uint64_t* at = reinterpret_cast<uint64_t*>(grid) + t;
    const uint64_t before = *at;
    uint64_t after = before;
#pragma unroll
    for (uint32_t k = 0; k < 8u; ++k) {
        if (l[k] == 0u || l[k] > K) continue;
        const bool keeps = rule == COMP_SELECT_LARGEST ? l[k] == bestNumber : keep[l[k] - 1u] != 0u;
        if (!keeps) after = (after & ~(0xffull << 8u * k)) | (of == COMP_EMPTY ? 1ull << 8u * k : 0ull);
    }
    if (after != before) *at = after;
}

static uint32_t comp_total(uint32_t N) { return N * N * N; }
static uint32_t comp_linear_words(uint32_t N) { return (comp_total(N) + 63u) / 64u; }

// scratch of one build: the member mask, the root bits and the roots in front of every 64 voxels, the scan's block sums, the total
size_t comp_scratch_bytes(uint32_t N)
{
    const size_t words = comp_linear_words(N);
    return align256(fill_mask_words(N) * sizeof(uint64_t)) + align256(words * sizeof(uint64_t)) + align256(words * sizeof(uint32_t)) +
           align256((size_t)scan_blocks(words) * sizeof(unsigned long long)) + align256(sizeof(unsigned long long));
}
void comp_scratch_layout(uint8_t* scratch, uint32_t N, CompParams& p)
{
    const size_t words = comp_linear_words(N);
    p.N = N;
    p.mask = reinterpret_cast<uint64_t*>(scratch);
    scratch += align256(fill_mask_words(N) * sizeof(uint64_t));
    p.rootMask = reinterpret_cast<uint64_t*>(scratch);
    scratch += align256(words * sizeof(uint64_t));
    p.bases = reinterpret_cast<uint32_t*>(scratch);
    scratch += align256(words * sizeof(uint32_t));
    p.sums = reinterpret_cast<unsigned long long*>(scratch);
    scratch += align256((size_t)scan_blocks(words) * sizeof(unsigned long long));
    p.total = reinterpret_cast<unsigned long long*>(scratch);
}

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
    k_comp_roots<<<(words + 3u) / 4u, 256, 0, s>>>(p.labels, total, p.rootMask, p.bases, words);
    const hipError_t e = launch_scan_words(p.bases, 1, words, p.sums, p.total, s);
    if (e != hipSuccess) return e;
    k_comp_number<<<(total / 4u + 255u) / 256u, 256, 0, s>>>(p.labels, total, p.rootMask, p.bases);
    return hipGetLastError();
}

// the table of the K components launch_comp_label found (K >= 1); p.stats: K CompStats of scratch
hipError_t launch_comp_stats(const CompParams& p, uint32_t K, hipStream_t s)
{
    if (!comp_params_ok(p) || !K || !p.stats || !p.table) return hipErrorInvalidValue;
    const uint32_t N = p.N, maskWords = N * N * fill_row_words(N), words = comp_linear_words(N);
    k_comp_stats_init<<<(K + 255u) / 256u, 256, 0, s>>>(p.stats, K);
    k_comp_first<<<(words + 255u) / 256u, 256, 0, s>>>(p.rootMask, p.bases, words, p.table, K);
    k_comp_stats<<<(maskWords + 255u) / 256u, 256, 0, s>>>(p.mask, N, p.labels, p.stats, maskWords, K);
    k_comp_table<<<(K + 255u) / 256u, 256, 0, s>>>(p.stats, p.table, K);
    return hipGetLastError();
}

size_t comp_select_bytes(uint32_t K) { return align256(4u * sizeof(unsigned long long)) + align256(K); }
unsigned long long* comp_select_counters(uint8_t* work) { return reinterpret_cast<unsigned long long*>(work); }

// the grid edited from its labels: `work` holds the four counters, then K keep flags
hipError_t launch_comp_select(uint8_t* grid, uint32_t N, int of, const uint32_t* labels, const CompRecord* table, uint32_t K, int rule, uint32_t arg, uint8_t* work,
                              hipStream_t s)
{
    if (N < 2u || N > kCompMaxN || (N & 1u) || !grid || !labels || !work || (K && !table)) return hipErrorInvalidValue;
    unsigned long long* counters = comp_select_counters(work);
    uint8_t* keep = work + align256(4u * sizeof(unsigned long long));
    const hipError_t e = hipMemsetAsync(counters, 0, 4u * sizeof(unsigned long long), s);
    if (e != hipSuccess) return e;
    if (!K) return hipSuccess;
    const uint32_t groups = comp_total(N) / 8u;
    k_comp_keep<<<(K + 255u) / 256u, 256, 0, s>>>(table, K, rule, arg, keep, counters);
    k_comp_edit<<<(groups + 255u) / 256u, 256, 0, s>>>(grid, labels, groups, of, rule, K, keep, counters);
    return hipGetLastError();
}

} // namespace dxv
