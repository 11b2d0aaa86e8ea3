// dxv_scratch.h -- how an operator's scratch memory is described: ONCE, by a function that takes its buffers one after the other from a Carve
// and stores the pointers in the operator's params.  Run over a null base the function gives the bytes to allocate (X_scratch_bytes), run over
// the allocation it gives the layout, and fits() says whether the allocation holds what was taken -- a caller that finds it does not refuses
// the call before anything is launched.  Host code without HIP: tests/hostcheck/scratch_check.cpp compiles every carve for the CPU.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace dxv {

// device allocations and the blocks inside one are laid out in whole 256-byte lines
inline size_t align256(size_t v) { return (v + 255) & ~size_t(255); }

struct Carve {
    uint8_t* base;
    size_t capacity, at = 0;
    Carve(void* b, size_t cap) : base(static_cast<uint8_t*>(b)), capacity(cap) {}
    // n bytes as they are: for the few blocks that are not whole lines
    uint8_t* take_bytes(size_t n)
    {
        uint8_t* p = base ? base + at : nullptr;
        at += n;
        return p;
    }
    // `count` elements in whole lines
    template <class T> T* take(size_t count) { return reinterpret_cast<T*>(take_bytes(align256(count * sizeof(T)))); }
    size_t used() const { return at; }
    bool fits() const { return at <= capacity; }
};

// element n of a block that was taken whole (the totals behind a block's sums): null stays null
template <class T> T* carve_at(T* block, size_t n) { return block ? block + n : nullptr; }

// what a carve function takes when nothing is allocated yet: fn(carve, args ..., params) -> the bytes
template <class P, class F, class... A> size_t carved_bytes(F fn, A... args)
{
    Carve c(nullptr, 0);
    P p{};
    fn(c, args..., p);
    return c.used();
}

// A record three operators keep per label in their work memory while their stats passes run (components, the skeleton's nodes, the partition's
// regions): the voxels, their box and their flags, gathered with 32-bit integer atomics -- a sum, minima, maxima, an OR: no arrival order shows
struct BoxStats { uint32_t voxels, lo[3], hi[3], flags; };
constexpr BoxStats box_stats_none() { return BoxStats{0u, {0xffffffffu, 0xffffffffu, 0xffffffffu}, {0u, 0u, 0u}, 0u}; }

// scan.hip: the words of one workgroup of launch_scan_words, and the block sums a scan of `words` words needs
constexpr uint32_t kScanWords = 1024;
inline uint32_t scan_blocks(size_t words) { return (uint32_t)((words + kScanWords - 1u) / kScanWords); }

// radix_sort.hip: the three shapes' limits, and the words of the histogram scratch of a sort of n keys, whatever its plan: bins x tiles + bins
// of the shape with the most of them
constexpr uint32_t kSortSmall = 2u << 20;           // up to here: tiles of 4 waves x 8 keys per lane, digits of up to 11 bits (fewest passes)
constexpr uint32_t kSortMedium = 16u << 20;         // up to here: tiles of 4 waves x 16 keys per lane, digits of 8 bits; beyond: 16 waves, 10 bits
inline uint32_t radix_sort_hist_words(uint32_t n)
{
    if (n <= kSortSmall) return 2048u * ((n + 2047u) / 2048u) + 2048u;
    if (n <= kSortMedium) return 2048u * ((n + 4095u) / 4096u) + 2048u;
    return 1024u * (uint32_t)(((uint64_t)n + 16383ull) / 16384ull) + 1024u;
}

} // namespace dxv
