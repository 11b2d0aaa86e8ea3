// The operators' scratch descriptions (the X_carve functions, through tests/hostcheck/scratch_check.cpp) in a program of their own, for a build
// with -fsanitize=address,undefined: every operator at the small sides and count pairs of tests/golden/operator_scratch.json is sized over no
// base, given an allocation of EXACTLY those bytes, carved over it, and the first and the last byte of every block it was handed are written --
// a block is what lies between one offset and the next, the last one ends with the allocation; blocks that share their words (parent and
// number, G and the centres) are one, a pointer at or behind the end belongs to a buffer of no elements.  A carve that hands out a byte it did
// not count is a heap overflow here.  Prints one line per operator; exits 0 when every carve fits its own size.
#include "../hostcheck/scratch_check.cpp"

#include <algorithm>
#include <cstdio>
#include <cstdlib>

static int touch(const char* op, std::vector<unsigned long long> args, unsigned long long& bytes)
{
    args.resize(4, 0ull);
    ScratchRow sized, laid;
    if (!scratch_row(op, args.data(), nullptr, 0, sized) || !sized.used) { fprintf(stderr, "%s: no size\n", op); return 1; }
    uint8_t* base = static_cast<uint8_t*>(malloc(sized.used));
    if (!base) { fprintf(stderr, "%s: no memory for %zu bytes\n", op, sized.used); return 1; }
    int bad = 0;
    if (!scratch_row(op, args.data(), base, sized.used, laid) || laid.used != sized.used || !laid.fits) { fprintf(stderr, "%s: sized %zu, laid out %zu\n", op, sized.used, laid.used); bad = 1; }
    ScratchRow shortOne;
    if (!bad && (!scratch_row(op, args.data(), base, sized.used - 1u, shortOne) || shortOne.fits)) { fprintf(stderr, "%s: fits one byte less\n", op); bad = 1; }
    std::vector<size_t> at;
    for (const auto& p : laid.at)
        if (p.second) at.push_back((size_t)(static_cast<const uint8_t*>(p.second) - base));
    std::sort(at.begin(), at.end());
    at.erase(std::unique(at.begin(), at.end()), at.end());
    while (!at.empty() && at.back() >= sized.used) at.pop_back();
    if (!bad && (at.empty() || at[0] != 0u)) { fprintf(stderr, "%s: nothing starts at the base\n", op); bad = 1; }
    for (size_t k = 0; !bad && k < at.size(); ++k) {
        const size_t end = k + 1u < at.size() ? at[k + 1u] : sized.used;
        base[at[k]] = (uint8_t)k;
        base[end - 1u] = (uint8_t)~k;
    }
    free(base);
    bytes += sized.used;
    return bad;
}

int main()
{
    const unsigned long long sides[] = {2, 4, 6, 8, 10, 14, 16, 18, 30, 32, 34, 62, 64, 66, 72};
    const unsigned long long pairs[][2] = {{0, 0}, {1, 0}, {0, 1}, {1, 1}, {255, 256}, {257, 100000}};
    const char* bySide[] = {"comp", "skel", "oct", "iso", "thick", "part", "geo", "fill", "thin", "dist"};
    for (const char* op : bySide) {
        unsigned long long bytes = 0;
        for (unsigned long long N : sides)
            if (touch(op, {N}, bytes)) return 1;
        printf("%s: %llu bytes\n", op, bytes);
    }
    unsigned long long bytes = 0;
    for (unsigned long long N : sides)
        for (unsigned long long intrusion = 0; intrusion < 2; ++intrusion)
            if (touch("access", {N, intrusion}, bytes)) return 1;
    printf("access: %llu bytes\n", bytes);
    bytes = 0;
    const unsigned long long radii[] = {1, 2, 9, 4096};
    for (unsigned long long N : sides)
        for (unsigned long long op = 0; op < 4; ++op)
            for (unsigned long long form = 1; form <= 2; ++form)
                for (unsigned long long r2 : radii)
                    if (touch("morph", {N, op, r2, form}, bytes)) return 1;
    printf("morph: %llu bytes\n", bytes);
    const char* byCount[] = {"part_work", "skel_prune", "comp_select"};
    for (const char* op : byCount) {
        bytes = 0;
        for (const auto& kb : pairs)
            if (touch(op, {kb[0], kb[1]}, bytes)) return 1;
        printf("%s: %llu bytes\n", op, bytes);
    }
    return 0;
}
