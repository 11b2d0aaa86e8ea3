// The product's skeleton routines (csrc/dxv_skeleton.h, with the union-find of csrc/dxv_components.h) compiled for the CPU: the same chain as
// csrc/skeleton.hip -- the member mask packed from the bytes, every word classified, the first parents over the node and curve masks, the merge
// over each mask at connectivity 26, every entry its root, the two kinds of roots ranked, the stats per run of node voxels and per curve voxel,
// the tables, and the prune from them -- with loops where the device has lanes, plain accesses where it has atomics.  tests/skeleton_host.py loads
// this; tests/test_skeleton_rule.py compares it with the restatements; tests/cpp/skeleton_sanitize_main.cpp includes it under the sanitizers.
#include <cstdint>
#include <cstring>
#include <vector>
#include "../../dxrvoxelizer_amd/csrc/dxv_skeleton.h"

using namespace dxv;

namespace {

struct PlainParent {
    uint32_t* p;
    uint32_t load(uint32_t i) const { return p[i]; }
    uint32_t lower(uint32_t i, uint32_t v) const { const uint32_t old = p[i]; if (v < old) p[i] = v; return old; }
};

struct Skeleton {
    uint32_t N = 0;
    std::vector<uint64_t> member, node, curve, ends;
    std::vector<uint32_t> labels;
    std::vector<SkelNode> nodes;
    std::vector<SkelBranch> branches;
    uint64_t counts[3] = {0, 0, 0};
};

void skeleton_of(const uint8_t* grid, uint32_t N, const uint32_t* weights, Skeleton& s)
{
    const uint32_t W = fill_row_words(N), total = N * N * N;
    const size_t words = fill_mask_words(N);
    s.N = N;
    s.member.assign(words, 0); s.node.assign(words, 0); s.curve.assign(words, 0); s.ends.assign(words, 0);
    for (size_t row = 0; row < (size_t)N * N; ++row)
        for (uint32_t j = 0; 8u * j < N; ++j) s.member[row * W + j / 8u] |= (uint64_t)comp_member_byte(grid + row * N, N, j, COMP_SOLID) << 8u * (j % 8u);
    for (uint32_t z = 0; z < N; ++z)
        for (uint32_t y = 0; y < N; ++y)
            for (uint32_t w = 0; w < W; ++w) {
                const size_t t = ((size_t)z * N + y) * W + w;
                if (!s.member[t]) continue;
                const SkelClass c = skel_classify_word(s.member.data(), N, y, z, w);
                s.node[t] = c.node; s.curve[t] = c.curve; s.ends[t] = c.ends;
                s.counts[0] += comp_popc(c.ends); s.counts[1] += comp_popc(c.curve); s.counts[2] += comp_popc(c.junctions);
            }
    s.labels.resize(total);
    for (uint32_t p = 0; p < total; ++p) s.labels[p] = skel_init_parent(s.node.data(), s.curve.data(), N, p);
    PlainParent par{s.labels.data()};
    for (const uint64_t* mask : {s.node.data(), s.curve.data()})
        for (uint32_t z = 0; z < N; ++z)
            for (uint32_t y = 0; y < N; ++y)
                for (uint32_t w = 0; w < W; ++w) comp_merge_word(par, mask, N, 26u, y, z, w);
    for (uint32_t p = 0; p < total; ++p)
        if (s.labels[p] != kCompNone) s.labels[p] = comp_root(par, p);
    // the roots in ascending order are the `first` of consecutive nodes and of consecutive branches
    std::vector<uint32_t> number(total, 0);
    std::vector<uint32_t> nodeFirst, branchFirst;
    for (uint32_t p = 0; p < total; ++p)
        if (s.labels[p] == p) {
            const bool branch = skel_bit(s.curve.data(), N, p);
            std::vector<uint32_t>& firsts = branch ? branchFirst : nodeFirst;
            firsts.push_back(p);
            number[p] = skel_label((uint32_t)firsts.size(), branch);
        }
    for (uint32_t p = 0; p < total; ++p) s.labels[p] = s.labels[p] == kCompNone ? 0u : number[s.labels[p]];
    const uint32_t K = (uint32_t)nodeFirst.size(), B = (uint32_t)branchFirst.size();
    std::vector<SkelNodeStats> stats(K);
    for (SkelNodeStats& st : stats) {
        st.voxels = st.degree = st.flags = st.w_max = 0u;
        for (int a = 0; a < 3; ++a) { st.lo[a] = 0xffffffffu; st.hi[a] = 0u; }
    }
    s.branches.assign(B, SkelBranch{});
    for (uint32_t b = 0; b < B; ++b) { s.branches[b].a = kCompNone; s.branches[b].w_min = 0xffffffffu; s.branches[b].first = branchFirst[b]; }
    auto lower = [](uint32_t& at, uint32_t v) { if (v < at) at = v; };
    auto raise = [](uint32_t& at, uint32_t v) { if (v > at) at = v; };
    for (uint32_t z = 0; z < N; ++z)
        for (uint32_t y = 0; y < N; ++y)
            for (uint32_t w = 0; w < W; ++w) {
                const size_t t = ((size_t)z * N + y) * W + w;
                const uint32_t base = (z * N + y) * N + 64u * w;
                const uint64_t e = s.ends[t];
                uint64_t m = s.node[t];
                while (m) {
                    uint32_t at, len;
                    comp_take_run(m, at, len);
                    SkelNodeStats& st = stats[s.labels[base + at] - 1u];
                    const uint32_t x0 = 64u * w + at, x1 = x0 + len - 1u;
                    const uint64_t run = (len == 64u ? ~0ull : (1ull << len) - 1ull) << at;
                    st.voxels += len;
                    lower(st.lo[0], x0); lower(st.lo[1], y); lower(st.lo[2], z);
                    raise(st.hi[0], x1); raise(st.hi[1], y); raise(st.hi[2], z);
                    st.flags |= (comp_run_flags(N, x0, x1, y, z) ? SKEL_NODE_BORDER : 0u) | ((run & e) ? SKEL_NODE_END : 0u) | ((run & ~e) ? SKEL_NODE_JUNCTION : 0u);
                    if (weights)
                        for (uint32_t k = 0; k < len; ++k) raise(st.w_max, weights[base + at + k]);
                }
                m = s.curve[t];
                while (m) {
                    uint32_t at, len;
                    comp_take_run(m, at, len);
                    SkelBranch& br = s.branches[(s.labels[base + at] & ~kSkelBranchBit) - 1u];
                    const uint32_t x0 = 64u * w + at, x1 = x0 + len - 1u;
                    br.voxels += len;
                    if (comp_run_flags(N, x0, x1, y, z)) br.flags |= SKEL_BRANCH_BORDER;
                    for (uint32_t k = 0; k < len; ++k) {
                        const uint32_t p = base + at + k;
                        if (weights) { lower(br.w_min, weights[p]); raise(br.w_max, weights[p]); br.w_sum += weights[p]; }
                        skel_neighbours(s.member.data(), s.curve.data(), N, y, z, w, at + k, [&](uint32_t q, int dx, int dy, int dz, bool isCurve) {
                            if (isCurve) {
                                if (p < q) ++br.steps[skel_step_type(dx, dy, dz)];
                                return;
                            }
                            ++br.steps[skel_step_type(dx, dy, dz)];
                            const uint32_t k2 = s.labels[q];
                            lower(br.a, k2); raise(br.b, k2);
                            ++stats[k2 - 1u].degree;
                        });
                    }
                }
            }
    s.nodes.resize(K);
    for (uint32_t k = 0; k < K; ++k) s.nodes[k] = skel_node_record(nodeFirst[k], stats[k]);
    for (SkelBranch& br : s.branches) skel_finish_branch(br, s.nodes.data(), weights != nullptr);
}

// the grid edited from a skeleton of it: {branches removed, voxels removed}
void prune_from(uint8_t* grid, const Skeleton& s, uint32_t maxLen345, uint64_t removed[2])
{
    std::vector<uint8_t> goB(s.branches.size(), 0), goN(s.nodes.size(), 0);
    removed[0] = removed[1] = 0;
    for (size_t b = 0; b < s.branches.size(); ++b) {
        const SkelBranch& r = s.branches[b];
        if (!skel_pruned(r, maxLen345)) continue;
        goB[b] = 1; goN[skel_spur_tip(r, s.nodes.data()) - 1u] = 1;
        ++removed[0]; removed[1] += (uint64_t)r.voxels + 1u;
    }
    for (size_t p = 0; p < s.labels.size(); ++p) {
        const uint32_t l = s.labels[p], number = l & ~kSkelBranchBit;
        if (number && ((l & kSkelBranchBit) ? goB[number - 1u] : goN[number - 1u])) grid[p] = 0;
    }
}

Skeleton g_last;

} // namespace

extern "C" {

// grid: N^3 bytes; weights: N^3 uint32 or NULL; counts: {K, B, end voxels, curve voxels, junction voxels}, written.  The skeleton stays with the
// library until the next call: sk_copy hands it out.
int sk_skeleton(const uint8_t* grid, uint32_t N, const uint32_t* weights, uint64_t* counts)
{
    if (!skel_valid(N)) return 1;
    g_last = Skeleton();
    skeleton_of(grid, N, weights, g_last);
    counts[0] = g_last.nodes.size(); counts[1] = g_last.branches.size();
    counts[2] = g_last.counts[0]; counts[3] = g_last.counts[1]; counts[4] = g_last.counts[2];
    return 0;
}
void sk_copy(uint32_t* labels, void* nodes, void* branches)
{
    memcpy(labels, g_last.labels.data(), g_last.labels.size() * sizeof(uint32_t));
    if (!g_last.nodes.empty()) memcpy(nodes, g_last.nodes.data(), g_last.nodes.size() * sizeof(SkelNode));
    if (!g_last.branches.empty()) memcpy(branches, g_last.branches.data(), g_last.branches.size() * sizeof(SkelBranch));
}
// the grid, in place, pruned from its own skeleton; removed: {branches, voxels}, written
int sk_prune(uint8_t* grid, uint32_t N, uint32_t maxLen345, uint64_t* removed)
{
    if (!skel_valid(N)) return 1;
    Skeleton s;
    skeleton_of(grid, N, nullptr, s);
    prune_from(grid, s, maxLen345, removed);
    return 0;
}
int sk_valid(uint32_t N) { return skel_valid(N) ? 1 : 0; }
uint32_t sk_max_n(void) { return kSkelMaxN; }

}
