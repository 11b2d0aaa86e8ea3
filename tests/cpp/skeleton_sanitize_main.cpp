// The product's skeleton routines (csrc/dxv_skeleton.h and the union-find of csrc/dxv_components.h, through tests/hostcheck/skeleton_check.cpp) in
// a program of their own, for a build with -fsanitize=address,undefined.  The grids: the builders' (tests/skeleton_restated.py: the figures, in
// the middle of the grid and at its corners, the word seams at 72 and 130, random grids, the contended grid), which the test writes into the file
// named on the command line -- per grid the side, then N^3 bytes --; and sparse and dense random grids at sides 2, 6, 10, 26 and 66: a side
// below a word, a row that ends inside its second word.  Every grid runs without and with weights and is pruned at three bounds.  What deg == 2
// promises must hold: steps = voxels + 1 and two attachments for a path, steps = voxels >= 3 for a cycle, the nodes' degrees sum to the
// attachments, every member has a label of its kind within 1 .. K or 1 .. B, and a prune removes what it says.  Prints one line per run; exits
// 0 when everything agrees.
#include "../hostcheck/skeleton_check.cpp"

#include <cstdio>

static uint32_t g_state = 2463534242u;
static uint32_t next() { return g_state = g_state * 1664525u + 1013904223u; }

static int run_grid(const char* what, uint32_t N, const std::vector<uint8_t>& g)
{
    const size_t n3 = (size_t)N * N * N;
    std::vector<uint32_t> weights(n3);
    for (uint32_t& w : weights) w = next() % 5u == 0u ? 0xFFFFFFFFu : next() % 4097u;
    for (int weighted = 0; weighted < 2; ++weighted) {
        Skeleton s;
        skeleton_of(g.data(), N, weighted ? weights.data() : nullptr, s);
        uint64_t members = 0, labelled = 0, attachments = 0, degrees = 0;
        for (size_t p = 0; p < n3; ++p) {
            const uint32_t l = s.labels[p], number = l & ~kSkelBranchBit;
            members += g[p] ? 1u : 0u;
            if ((l != 0u) != (g[p] != 0) || number > ((l & kSkelBranchBit) ? s.branches.size() : s.nodes.size())) { fprintf(stderr, "%s N %u: the label of voxel %zu\n", what, N, p); return 1; }
            labelled += l ? 1u : 0u;
        }
        if (members != labelled || s.counts[0] + s.counts[1] + s.counts[2] != members) { fprintf(stderr, "%s N %u: %llu members\n", what, N, (unsigned long long)members); return 1; }
        uint64_t voxels = 0;
        for (const SkelBranch& r : s.branches) {
            const uint64_t steps = (uint64_t)r.steps[0] + r.steps[1] + r.steps[2];
            const bool closed = (r.flags & SKEL_BRANCH_CLOSED) != 0u;
            if (closed ? (r.a || r.b || steps != r.voxels || r.voxels < 3u) : (!r.a || r.a > r.b || r.b > s.nodes.size() || steps != (uint64_t)r.voxels + 1u)) {
                fprintf(stderr, "%s N %u: a branch of %u voxels and %llu steps\n", what, N, r.voxels, (unsigned long long)steps);
                return 1;
            }
            if (weighted ? (r.w_min > r.w_max || r.w_sum < r.w_max) : (r.w_min || r.w_max || r.w_sum)) return 1;
            attachments += closed ? 0u : 2u;
            voxels += r.voxels;
        }
        for (const SkelNode& n : s.nodes) { degrees += n.degree; voxels += n.voxels; }
        if (degrees != attachments || voxels != members || voxels - s.counts[1] != s.counts[0] + s.counts[2]) { fprintf(stderr, "%s N %u: degrees %llu, attachments %llu\n", what, N, (unsigned long long)degrees, (unsigned long long)attachments); return 1; }
        const uint32_t bounds[] = {0u, 12u, 0xFFFFFFFFu};
        for (uint32_t bound : bounds) {
            std::vector<uint8_t> edited(g);
            uint64_t removed[2], gone = 0;
            if (sk_prune(edited.data(), N, bound, removed)) return 1;
            for (size_t p = 0; p < n3; ++p) {
                if (edited[p] != g[p] && edited[p] != 0) return 1;
                gone += edited[p] != g[p] ? 1u : 0u;
            }
            if (gone != removed[1] || (bound == 0u && gone)) { fprintf(stderr, "%s N %u: a prune at %u removed %llu voxels and reports %llu\n", what, N, bound, (unsigned long long)gone, (unsigned long long)removed[1]); return 1; }
        }
        printf("%s N %u weights %d: nodes %zu branches %zu ends %llu curve %llu junctions %llu\n", what, N, weighted, s.nodes.size(), s.branches.size(), (unsigned long long)s.counts[0],
               (unsigned long long)s.counts[1], (unsigned long long)s.counts[2]);
    }
    return 0;
}

int main(int argc, char** argv)
{
    if (argc != 2) { fprintf(stderr, "usage: %s builders.bin\n", argv[0]); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
    uint32_t N = 0, builders = 0;
    while (fread(&N, sizeof(uint32_t), 1, f) == 1) {
        if (!skel_valid(N) || N > 130u) { fprintf(stderr, "a builder of side %u\n", N); return 2; }
        std::vector<uint8_t> g((size_t)N * N * N);
        if (fread(g.data(), 1, g.size(), f) != g.size()) { fprintf(stderr, "a short builder\n"); return 2; }
        if (run_grid("builder", N, g)) return 1;
        ++builders;
    }
    fclose(f);
    if (!builders) { fprintf(stderr, "no builder in %s\n", argv[1]); return 2; }
    const uint32_t sides[] = {2u, 6u, 10u, 26u, 66u};
    for (uint32_t side : sides)
        for (uint32_t density = 1; density <= 4u; density += 3u) {
            std::vector<uint8_t> g((size_t)side * side * side);
            for (uint8_t& v : g) v = next() % 20u < density ? (uint8_t)(1u + next() % 255u) : 0;
            if (run_grid(density == 1u ? "sparse" : "dense", side, g)) return 1;
        }
    uint64_t counts[5];
    std::vector<uint8_t> one(27, 1);
    if (sk_skeleton(one.data(), 3u, nullptr, counts) != 1 || sk_valid(1026u) || !sk_valid(1024u)) { fprintf(stderr, "a side that is not valid accepted\n"); return 1; }
    return 0;
}
