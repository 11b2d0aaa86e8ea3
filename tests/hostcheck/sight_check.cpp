// The product's line-of-sight routines (csrc/dxv_sight.h) compiled for the CPU: the same chain as csrc/sight.hip -- the grid packed into the
// member mask, every requested direction swept into its plane word by word, the map composed from the planes' words, the tally from the words
// -- with loops where the device has lanes.  A row group of the sweep is an array of `group` words that step together: every word's carry is
// taken from the word beside it as it stood BEFORE the step, the way the device's shuffle hands it over, the group's spare words included.
// Mask, planes and the tally's words lie where sight_carve puts them, in an allocation of exactly sight_scratch_bytes.
// tests/sight_host.py loads this; tests/test_sight_rule.py compares it with the restatements.
#include <cstring>
#include <vector>

#include "../../dxrvoxelizer_amd/csrc/dxv_sight.h"

using namespace dxv;

// k_sight_pack
static void sc_pack(const uint8_t* grid, uint32_t N, int of, uint64_t* mask)
{
    const uint32_t rowBytes = fill_row_words(N) * 8u;
    uint8_t* bytes = reinterpret_cast<uint8_t*>(mask);
    for (size_t t = 0; t < (size_t)N * N * rowBytes; ++t) {
        const size_t row = t / rowBytes;
        const uint32_t j = (uint32_t)(t % rowBytes);
        uint32_t bits = 0;
        if (8u * j < N) {
            const uint8_t* g = grid + row * N;
            if (N & 7u) bits = sight_member_byte(g, N, j, of);
            else {
                uint64_t eight;
                memcpy(&eight, g + 8u * j, 8);
                bits = sight_member_byte(eight, of);
            }
        }
        bytes[t] = (uint8_t)bits;
    }
}

// k_sight_sweep for one direction: a group of G words per family, stepping together
static void sc_sweep(const uint64_t* mask, uint32_t N, uint32_t b, uint32_t G, uint64_t* plane)
{
    const uint32_t W = fill_row_words(N);
    const SightSweep s = sight_sweep(b, N);
    if (s.axis == 0) {
        for (uint32_t row = 0; row < s.families; ++row) sight_row_x(mask + (size_t)row * W, plane + (size_t)row * W, N, W, s.dx);
        return;
    }
    std::vector<uint64_t> V(G);
    std::vector<uint32_t> carry(G);
    for (uint32_t f = 0; f < s.families; ++f) {
        for (uint64_t& v : V) v = ~0ull;
        for (uint32_t k = 0; k < N; ++k) {
            for (uint32_t w = 0; w < G; ++w) carry[w] = sight_carry(V[w], s.dx);
            const int32_t row = sight_row_at(s, N, f, k);
            for (uint32_t w = 0; w < G; ++w) {
                // __shfl_up / __shfl_down by one inside the group: the group's first / last lane reads itself
                const uint32_t in = s.dx > 0 ? carry[w ? w - 1u : w] : s.dx < 0 ? carry[w + 1u < G ? w + 1u : w] : carry[w];
                if ((uint32_t)row >= N) { V[w] = ~0ull; continue; }
                const size_t at = (size_t)sight_step_at(s, N, k) * s.stepStride + (size_t)row * s.rowStride + w;
                V[w] = sight_step(w < W ? mask[at] : 0ull, V[w], in, s.dx, N, w, W);
                if (w < W) plane[at] = V[w];
            }
        }
    }
}

extern "C" {

uint32_t sc_max_n() { return kSightMaxN; }
uint32_t sc_all() { return kSightAll; }
uint32_t sc_bit(int dx, int dy, int dz) { return sight_bit(dx, dy, dz); }
int sc_valid(uint32_t N, int of, uint32_t directions) { return sight_valid(N, of, directions) ? 1 : 0; }
uint32_t sc_group(uint32_t W, uint32_t atLeast) { return sight_group(W, atLeast); }

// the carve over `capacity` bytes at `base` (0: the sizing run): the bytes taken, whether they fit, and where the three blocks begin
uint64_t sc_carve(uint32_t N, uint32_t directions, uint64_t base, uint64_t capacity, int* fits, uint64_t offsets[3])
{
    Carve c(reinterpret_cast<void*>(base), capacity);
    SightScratch l{};
    sight_carve(c, N, directions, l);
    *fits = c.fits() ? 1 : 0;
    offsets[0] = reinterpret_cast<uint64_t>(l.tally); offsets[1] = reinterpret_cast<uint64_t>(l.mask); offsets[2] = reinterpret_cast<uint64_t>(l.planes);
    return c.used() == sight_scratch_bytes(N, directions) ? c.used() : 0u;
}

// map: N^3 words; tally: 68.  group: option sightgroup.  0, or 1 where the device refuses
int sc_sight(const uint8_t* grid, uint32_t N, int of, uint32_t directions, uint32_t group, uint32_t* map, uint64_t* tally)
{
    if (!sight_valid(N, of, directions) || group > kSightMaxGroup || (group & (group - 1u))) return 1;
    std::vector<uint8_t> scratch(sight_scratch_bytes(N, directions));
    Carve carve(scratch.data(), scratch.size());
    SightScratch l{};
    sight_carve(carve, N, directions, l);
    if (!carve.fits()) return 2;
    const uint32_t W = fill_row_words(N), words = N * N * W, G = sight_group(W, group), count = sight_popc(directions);
    memset(l.tally, 0, kSightTallyWords * sizeof(unsigned long long));
    sc_pack(grid, N, of, l.mask);
    uint32_t p = 0;
    for (uint32_t left = directions; left; left &= left - 1u, ++p) sc_sweep(l.mask, N, sight_lowest(left), G, l.planes + (size_t)p * words);
    if (p != count) return 3;
    SightTally total{};
    for (uint32_t u = 0; u < words; ++u) {
        uint64_t v[kSightBits];
        p = 0;
        for (uint32_t b = 0; b < kSightBits; ++b) v[b] = (directions >> b & 1u) ? l.planes[(size_t)p++ * words + u] : 0ull;
        const uint32_t row = u / W, w = u - row * W;
        for (uint32_t bit = 0; bit < 64u && w * 64u + bit < N; ++bit) map[(size_t)row * N + w * 64u + bit] = sight_map_word(v, bit);
        SightTallyOf<uint32_t> share{};                                 // (a thread's share, as the device keeps it)
        sight_tally_word(share, l.mask[u], v, directions);
        sight_tally_combine(total, share);
    }
    memcpy(l.tally, &total, sizeof(total));
    memcpy(tally, l.tally, sizeof(total));
    // both ends of every block, over an allocation of exactly the carve's size (the sanitizer program's run says whether that was inside)
    volatile uint64_t* ends[6] = {l.planes, l.planes + (size_t)count * words - 1u, l.mask, l.mask + words - 1u, reinterpret_cast<uint64_t*>(l.tally),
                                  reinterpret_cast<uint64_t*>(l.tally) + kSightTallyWords - 1u};
    for (volatile uint64_t* end : ends) *end = *end;
    return 0;
}

// k_sight_fill
int sc_sight_fill(uint8_t* grid, uint32_t N, int of, uint32_t directions, const uint32_t* map)
{
    if (!sight_valid(N, of, directions)) return 1;
    for (size_t v = 0; v < (size_t)N * N * N; ++v)
        if (sight_fill_changes(grid[v], map[v], of, directions)) grid[v] = sight_fill_byte(of);
    return 0;
}

} // extern "C"
