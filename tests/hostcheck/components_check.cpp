// The product's connected-component routines (dxrvoxelizer_amd/csrc/dxv_components.h) compiled for the CPU: the same text the kernels of
// components.hip run, driven here single-threaded in the kernels' order -- pack, init, merge word by word, compress, number, stats, table --
// with plain accesses behind the parent policy; and the select rules on a table.
#include "../../dxrvoxelizer_amd/csrc/dxv_components.h"

#include <string.h>
#include <vector>

using namespace dxv;

namespace {
struct PlainParent {
    uint32_t* p;
    uint32_t load(uint32_t i) const { return p[i]; }
    uint32_t lower(uint32_t i, uint32_t v) const
    {
        const uint32_t old = p[i];
        if (v < old) p[i] = v;
        return old;
    }
};
}

// grid: N^3 bytes; labels: N^3 uint32 out; table: room for N^3 records of 24 bytes out (or NULL: count only).  eightAtOnce != 0: the pack
// takes the 8-byte path where the kernel takes it (N % 8 == 0).  backwards != 0: the merge visits the words in descending order (the result
// does not depend on the order the unions arrive in).  Returns K, or -1 for arguments the library refuses.
extern "C" long long cc_components(const uint8_t* grid, uint32_t N, int of, uint32_t connectivity, int eightAtOnce, int backwards, uint32_t* labels, void* table)
{
    if (N < 2 || N > kCompMaxN || (N & 1u) || (of != COMP_SOLID && of != COMP_EMPTY) || (connectivity != 6 && connectivity != 26)) return -1;
    const uint32_t W = fill_row_words(N), rowBytes = W * 8u, total = N * N * N, linearWords = (total + 63u) / 64u;
    const size_t rows = (size_t)N * N;
    std::vector<uint64_t> mask(fill_mask_words(N));
    uint8_t* mb = reinterpret_cast<uint8_t*>(mask.data());
    const bool eight = eightAtOnce && (N & 7u) == 0u;
    for (size_t row = 0; row < rows; ++row)
        for (uint32_t j = 0; j < rowBytes; ++j) {
            uint32_t bits = 0;
            const uint8_t* g = grid + row * N;
            if (8u * j < N) {
                if (eight) {
                    uint64_t v;
                    memcpy(&v, g + 8u * j, 8);
                    bits = comp_member_byte(v, of);
                } else bits = comp_member_byte(g, N, j, of);
            }
            mb[row * rowBytes + j] = (uint8_t)bits;
        }
    for (uint32_t p = 0; p < total; ++p) labels[p] = comp_init_parent(mask.data(), N, p);
    PlainParent par{labels};
    const uint32_t maskWords = (uint32_t)(rows * W);
    for (uint32_t i = 0; i < maskWords; ++i) {
        const uint32_t t = backwards ? maskWords - 1u - i : i, row = t / W;
        comp_merge_word(par, mask.data(), N, connectivity, row % N, row / N, t - row * W);
    }
    for (uint32_t p = 0; p < total; ++p)
        if (labels[p] != kCompNone) labels[p] = comp_root(par, p);
    std::vector<uint64_t> rootMask(linearWords, 0);
    std::vector<uint32_t> bases(linearWords, 0);
    for (uint32_t p = 0; p < total; ++p)
        if (labels[p] == p) rootMask[p >> 6] |= 1ull << (p & 63u);
    uint32_t K = 0;
    for (uint32_t w = 0; w < linearWords; ++w) { bases[w] = K; K += comp_popc(rootMask[w]); }
    for (uint32_t p = 0; p < total; ++p) labels[p] = labels[p] == kCompNone ? 0u : comp_rank(rootMask.data(), bases.data(), labels[p]) + 1u;
    if (!table) return K;
    std::vector<CompStats> stats(K);
    std::vector<uint32_t> first(K);
    for (auto& s : stats) { s.voxels = 0; s.flags = 0; for (int a = 0; a < 3; ++a) { s.lo[a] = 0xffffffffu; s.hi[a] = 0; } }
    for (uint32_t w = 0; w < linearWords; ++w) {
        uint64_t roots = rootMask[w];
        for (uint32_t k = bases[w]; roots; ++k, roots &= roots - 1ull) first[k] = w * 64u + comp_ctz(roots);
    }
    for (uint32_t t = 0; t < maskWords; ++t) {
        const uint32_t row = t / W, w = t - row * W, y = row % N, z = row / N, base = row * N + 64u * w;
        uint64_t m = mask[t];
        while (m) {
            uint32_t s, len;
            comp_take_run(m, s, len);
            CompStats& st = stats[labels[base + s] - 1u];
            const uint32_t x0 = 64u * w + s, x1 = x0 + len - 1u, v[3] = {x0, y, z}, u[3] = {x1, y, z};
            st.voxels += len;
            for (int a = 0; a < 3; ++a) { if (v[a] < st.lo[a]) st.lo[a] = v[a]; if (u[a] > st.hi[a]) st.hi[a] = u[a]; }
            st.flags |= comp_run_flags(N, x0, x1, y, z);
        }
    }
    CompRecord* out = static_cast<CompRecord*>(table);
    for (uint32_t k = 0; k < K; ++k) out[k] = comp_record(first[k], stats[k]);
    return K;
}

// keep[k] = 1 / 0 for the K records of a table under a select rule; returns the number kept
extern "C" uint32_t cc_select(const void* table, uint32_t K, int rule, uint32_t arg, uint8_t* keep)
{
    const CompRecord* t = static_cast<const CompRecord*>(table);
    unsigned long long best = 0;
    for (uint32_t k = 0; k < K; ++k) {
        const unsigned long long key = comp_best_key(t[k].voxels, k + 1u);
        if (key > best) best = key;
    }
    uint32_t kept = 0;
    for (uint32_t k = 0; k < K; ++k) {
        keep[k] = comp_keep(rule, arg, k + 1u, t[k].voxels, t[k].flags, best) ? 1u : 0u;
        kept += keep[k];
    }
    return kept;
}

extern "C" uint32_t cc_run_start(uint64_t m, uint32_t b) { return comp_run_start(m, b); }
extern "C" uint32_t cc_max_n(void) { return kCompMaxN; }
