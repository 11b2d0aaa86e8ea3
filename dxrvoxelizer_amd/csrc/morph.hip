// morph.hip -- dilation, erosion, opening and closing of a whole N^3 grid by the exact Euclidean ball (dxv_morph.h has the rule and the word
// routines), in place, on the frame's stream.  A fixed number of kernels, nothing for the host to settle.  Two forms of the same bytes
// (dxv_morph.h: morph_form): up to kMorphPlanesMaxRadiusSq the planes,
//   k_morph_pack     grid (1 B per voxel) -> the member mask M (1 bit per voxel, the fill's layout; the complement inside the grid for ERODE and
//                    OPEN) and one bit per eight voxels "a byte here is neither 0 nor 1": the one read of the grid
//   k_morph_spread   per half: a mask -> its R planes, plane k = the mask spread by k along x; one lane per word, the row's two neighbour words
//   k_morph_ball     per half: the planes -> the dilated mask, one lane per word, one load and one OR per (dy, dz) of the disc; complemented
//                    inside the grid where the half asks for it.  OPEN and CLOSE run spread and ball twice and stay in bits in between.
//   k_morph_write    M and the result -> bytes 0 / 1, eight voxels per thread, a store only where one of the eight changes; voxels set and
//                    cleared are counted per wave and added with one atomic each: the one write of the grid
// and above it, where the planes would cost more than the distance field they replace, per half that field (distance.hip) and
//   k_morph_threshold  field and grid -> bytes 0 / 1 in place, eight voxels per thread, a store only where a byte changes, the same counters
// Lanes of a wave sit on adjacent words -- adjacent x, then adjacent y -- in every kernel, and the offsets of the ball are the same in every
// lane, so every load and store is a whole-wave access of consecutive words.  No loop waits for another workgroup, every loop is bounded
// by the radius; no LDS, no scratch memory.  The counters and either form's buffers are laid out by morph_carve (dxv_morph.h).
#include "dxv_device.h"
#include "dxv_morph.h"

namespace dxv {

// one thread per byte of a mask row (W * 8 of them, the ones behind the row's end are 0); every lane stays for the ballot
__global__ __launch_bounds__(256) void k_morph_pack(const uint8_t* __restrict__ grid, uint32_t N, int complement, uint8_t* __restrict__ mask, uint64_t* __restrict__ loose)
{
    const uint32_t rowBytes = fill_row_words(N) * 8u;
    const size_t t = (size_t)blockIdx.x * 256u + threadIdx.x;
    const bool in = t < (size_t)N * N * rowBytes;
    uint32_t bits = 0;
    bool odd = false;
    if (in) {
        const size_t row = t / rowBytes;
        const uint32_t j = (uint32_t)(t % rowBytes);
        if (8u * j < N) {
            const uint8_t* g = grid + row * N;
            if (N & 7u) { bits = morph_member_byte(g, N, j, complement != 0); odd = morph_loose(g, N, j); }
            else {
                const uint64_t eight = *reinterpret_cast<const uint64_t*>(g + 8u * j);
                bits = morph_member_byte(eight, complement != 0); odd = morph_loose(eight);
            }
        }
        mask[t] = (uint8_t)bits;
    }
    const uint64_t any = __ballot(odd);
    if (in && (threadIdx.x & 63u) == 0u) loose[t >> 6] = any;
}

__global__ __launch_bounds__(256) void k_morph_spread(const uint64_t* __restrict__ mask, uint32_t N, uint32_t R, uint64_t* __restrict__ planes, uint32_t words)
{
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    if (t >= words) return;
    const uint32_t W = fill_row_words(N), w = t % W;
    const uint64_t m = mask[t], prev = w ? mask[t - 1u] : 0ull, next = w + 1u < W ? mask[t + 1u] : 0ull;
    uint64_t cur = m;
    for (uint32_t k = 1; k <= R; ++k) {
        cur |= morph_shifted(prev, m, next, k);
        planes[(size_t)(k - 1u) * words + t] = cur;
    }
}

__global__ __launch_bounds__(256) void k_morph_ball(const uint64_t* __restrict__ mask, const uint64_t* __restrict__ planes, uint32_t N, uint32_t r2, int complement,
                                                    uint64_t* __restrict__ out, uint32_t words)
{
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    if (t >= words) return;
    const uint32_t W = fill_row_words(N), row = t / W, w = t - row * W;
    const uint64_t acc = morph_ball_word(mask, planes, words, N, W, r2, row % N, row / N, t);
    out[t] = (complement ? ~acc : acc) & morph_valid(N, w);
}

// was: the members the pack made (the complement of the solid where wasComplement); now: the result, the solid voxels.  counters: {set, cleared}
__global__ __launch_bounds__(256) void k_morph_write(const uint8_t* __restrict__ was, int wasComplement, const uint8_t* __restrict__ now, const uint64_t* __restrict__ loose,
                                                     uint32_t N, uint8_t* __restrict__ grid, unsigned long long* counters)
{
    const uint32_t rowBytes = fill_row_words(N) * 8u;
    const size_t t = (size_t)blockIdx.x * 256u + threadIdx.x;
    uint32_t set = 0, cleared = 0;
    if (t < (size_t)N * N * rowBytes) {
        const size_t row = t / rowBytes;
        const uint32_t j = (uint32_t)(t % rowBytes);
        if (8u * j < N) {
            const uint32_t left = N - 8u * j, valid = left >= 8u ? 0xffu : (1u << left) - 1u;
            const uint32_t before = (wasComplement ? ~(uint32_t)was[t] : (uint32_t)was[t]) & valid, after = now[t] & valid;
            set = morph_popc8(after & ~before);
            cleared = morph_popc8(before & ~after);
            if (before != after || ((loose[t >> 6] >> (t & 63u)) & 1ull)) {
                uint8_t* g = grid + row * N + 8u * j;
                if ((N & 7u) == 0u) *reinterpret_cast<uint64_t*>(g) = fill_spread_byte(after);
                else
                    for (uint32_t k = 0; k < 8u && k < left; ++k) g[k] = (uint8_t)((after >> k) & 1u);
            }
        }
    }
#pragma unroll
    for (uint32_t d = 1; d < 64u; d <<= 1) {                            // (every lane of the wave is here)
        set += (uint32_t)__shfl_xor((int)set, (int)d);
        cleared += (uint32_t)__shfl_xor((int)cleared, (int)d);
    }
    if ((threadIdx.x & 63u) == 0u) {
        if (set) (void)__hip_atomic_fetch_add(counters + 0, (unsigned long long)set, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (cleared) (void)__hip_atomic_fetch_add(counters + 1, (unsigned long long)cleared, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// ---- the field form: eight consecutive voxels per thread (linear order: N^3 is a multiple of 8), two 16-byte loads of the field, one 8-byte
// load of the grid, a store only where a byte changes.  second: the second half of OPEN / CLOSE, which can only take back what the first
// half did -- OPEN never sets and CLOSE never clears a voxel of the original grid --, so its counts come OFF the other counter. ----
__global__ __launch_bounds__(256) void k_morph_threshold(uint8_t* grid, const int32_t* __restrict__ field, uint32_t groups, uint32_t r2, int erode, int second,
                                                         unsigned long long* counters)
{
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    uint32_t set = 0, cleared = 0;
    if (t < groups) {
        const int4 a = reinterpret_cast<const int4*>(field)[2u * (size_t)t], b = reinterpret_cast<const int4*>(field)[2u * (size_t)t + 1u];
        const int32_t d[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
        uint64_t* at = reinterpret_cast<uint64_t*>(grid) + t;
        const uint64_t before = *at;
        uint32_t bits = 0;
#pragma unroll
        for (uint32_t k = 0; k < 8u; ++k) bits |= morph_threshold(d[k], r2, erode != 0) << k;
        const uint32_t was = solid_bits(before);
        set = morph_popc8(bits & ~was);
        cleared = morph_popc8(was & ~bits);
        const uint64_t after = fill_spread_byte(bits);
        if (after != before) *at = after;
    }
#pragma unroll
    for (uint32_t d = 1; d < 64u; d <<= 1) {                            // (every lane of the wave is here)
        set += (uint32_t)__shfl_xor((int)set, (int)d);
        cleared += (uint32_t)__shfl_xor((int)cleared, (int)d);
    }
    if ((threadIdx.x & 63u) == 0u) {
        // (unsigned: what the second half takes off never exceeds what the first half put there)
        if (set) (void)__hip_atomic_fetch_add(counters + (second ? 1 : 0), second ? 0ull - set : (unsigned long long)set, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (cleared) (void)__hip_atomic_fetch_add(counters + (second ? 0 : 1), second ? 0ull - cleared : (unsigned long long)cleared, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// pack and write-back for another operator on bit masks (thin.hip): the same two kernels, launched on its stream with its buffers
void launch_morph_pack(const uint8_t* grid, uint32_t N, uint8_t* mask, uint64_t* loose, hipStream_t s)
{
    k_morph_pack<<<(uint32_t)((fill_mask_words(N) * 8u + 255u) / 256u), 256, 0, s>>>(grid, N, 0, mask, loose);
}
void launch_morph_write(const uint8_t* was, const uint8_t* now, const uint64_t* loose, uint32_t N, uint8_t* grid, unsigned long long* counters, hipStream_t s)
{
    k_morph_write<<<(uint32_t)((fill_mask_words(N) * 8u + 255u) / 256u), 256, 0, s>>>(was, 0, now, loose, N, grid, counters);
}

static hipError_t launch_morph_field(uint8_t* grid, uint32_t N, int op, uint32_t r2, const MorphScratch& l, hipStream_t s)
{
    const uint32_t groups = (uint32_t)((size_t)N * N * N / 8u);
    for (uint32_t half = 0; half < morph_halves(op); ++half) {
        const hipError_t e = launch_distance(grid, N, 0, l.field, l.passes, s);
        if (e != hipSuccess) return e;
        k_morph_threshold<<<(groups + 255u) / 256u, 256, 0, s>>>(grid, l.field, groups, r2, morph_half_erodes(op, half) ? 1 : 0, (int)half, l.counters);
    }
    return hipGetLastError();
}

// l: morph_carve(N, op, r2, form) over the call's scratch
hipError_t launch_morph(uint8_t* grid, uint32_t N, int op, uint32_t r2, int form, const MorphScratch& l, hipStream_t s)
{
    if (!grid || !l.counters || N < 2u || N > kMorphMaxN || (N & 1u) || op < MORPH_DILATE || op > MORPH_CLOSE || r2 < 1u || r2 > kMorphMaxRadiusSq ||
        (form != MORPH_FORM_PLANES && form != MORPH_FORM_FIELD) || (form == MORPH_FORM_FIELD ? !l.field || !l.passes : !l.packed || !l.loose || !l.planes))
        return hipErrorInvalidValue;
    const hipError_t e = hipMemsetAsync(l.counters, 0, 2u * sizeof(unsigned long long), s);
    if (e != hipSuccess) return e;
    if (form == MORPH_FORM_FIELD) return launch_morph_field(grid, N, op, r2, l, s);
    const uint32_t W = fill_row_words(N), words = N * N * W, R = morph_isqrt(r2), halves = morph_halves(op);     // (N <= kMorphMaxN: 2^27 words at the most)
    const size_t maskBytes = (size_t)words * 8u;
    const uint32_t byteBlocks = (uint32_t)((maskBytes + 255u) / 256u), wordBlocks = (words + 255u) / 256u;
    const bool complement = morph_packs_complement(op);
    k_morph_pack<<<byteBlocks, 256, 0, s>>>(grid, N, complement ? 1 : 0, reinterpret_cast<uint8_t*>(l.packed), l.loose);
    const uint64_t* from = l.packed;
    for (uint32_t half = 0; half < halves; ++half) {
        k_morph_spread<<<wordBlocks, 256, 0, s>>>(from, N, R, l.planes, words);
        k_morph_ball<<<wordBlocks, 256, 0, s>>>(from, l.planes, N, r2, morph_half_complements(op, half) ? 1 : 0, l.half[half], words);
        from = l.half[half];
    }
    k_morph_write<<<byteBlocks, 256, 0, s>>>(reinterpret_cast<const uint8_t*>(l.packed), complement ? 1 : 0, reinterpret_cast<const uint8_t*>(from), l.loose, N, grid, l.counters);
    return hipGetLastError();
}

} // namespace dxv
