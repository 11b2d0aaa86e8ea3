// thin.hip -- topology-preserving thinning of a whole N^3 grid (dxv_thin.h has the rule and the word routines), in place, on the frame's stream:
//   pack            morph.hip's: grid (1 B per voxel) -> the solid mask S (1 bit per voxel, the fill's layout) and one bit per eight voxels "a
//                   byte here is neither 0 nor 1": the one read of the grid.  S is kept twice: as it was, and as the iterations leave it
//   k_thin_border   once per iteration: S -> the border mask B, one lane per word, its row's two neighbour words and the four words at y -+ 1, z -+ 1
//   k_thin_sub      once per sub-iteration s = 0 .. 7: lanes sit on the words of the rows with (y & 1, z & 1) of s, a quarter of the rows; a lane's
//                   candidates are the bits of B & S of s's x parity; the nine row triples round the word are loaded once, every candidate is
//                   decided from registers, one store covers the word if a bit went
//   write-back      morph.hip's: S as it was and as it is -> bytes 0 / 1, a store only where one of eight bytes changes or was loose
// k_thin_sub works IN PLACE on S, with no second mask and no atomics on it:
//   * every bit a lane reads for USE -- the 26 voxels round a candidate -- belongs to another subfield than the candidate's (two voxels of one
//     subfield differ by an even amount in every coordinate, so they are never 26-adjacent), and only bits of the launch's own subfield change in
//     this launch: whichever of the old and the new word a load returns, the bits looked at are the same;
//   * a word is stored by one lane only, the one that sits on it;
//   * an aligned 8-byte load or store does not tear.
// So S is neither const nor __restrict__ here: the loads may not be hoisted into a cache that is not coherent with this launch's stores.
// A batch is `iterations` iterations behind one another, nine launches each.  Whether an iteration removed a voxel is word `iteration` of the
// batch's control block; the kernels of an iteration return at once when the iteration before left its word 0, so a batch costs what its live
// iterations cost, and the host reads the block where the frame is next synchronised (dxv_products.hip: settle_thin).  No workgroup waits
// for another, every loop is bounded by 64 candidates and 26 flood steps; no LDS, no scratch memory.  The control block and the masks are laid
// out by thin_carve (dxv_thin.h).
#include "dxv_device.h"
#include "dxv_thin.h"

namespace dxv {

__global__ __launch_bounds__(256) void k_thin_border(const uint64_t* __restrict__ S, uint32_t N, uint64_t* __restrict__ B, uint32_t words, const ThinControl* ctl, uint32_t iteration)
{
    if (iteration && ctl->live[iteration - 1u] == 0u) return;
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    if (t >= words) return;
    const uint32_t W = fill_row_words(N), row = t / W, w = t - row * W, y = row % N, z = row / N;
    const size_t yStride = W, zStride = (size_t)N * W;
    B[t] = thin_border_word(S[t], w ? S[t - 1u] : 0ull, w + 1u < W ? S[t + 1u] : 0ull, y ? S[t - yStride] : 0ull, y + 1u < N ? S[t + yStride] : 0ull,
                            z ? S[t - zStride] : 0ull, z + 1u < N ? S[t + zStride] : 0ull);
}

__global__ __launch_bounds__(256) void k_thin_sub(uint64_t* S, const uint64_t* __restrict__ B, uint32_t N, uint32_t sub, int kind, uint32_t lanes, ThinControl* ctl,
                                                  uint32_t iteration)
{
    if (iteration && ctl->live[iteration - 1u] == 0u) return;
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    uint32_t gone = 0;
    if (t < lanes) {
        const uint32_t W = fill_row_words(N), half = N >> 1, w = t % W, r = t / W;
        const uint32_t y = 2u * (r % half) + ((sub >> 1) & 1u), z = 2u * (r / half) + ((sub >> 2) & 1u);
        const size_t at = ((size_t)z * N + y) * W + w;
        const uint64_t s = S[at], border = B[at];
        if (s & border & thin_x_parity(sub & 1u)) {
            ThinRow rows[9];
#pragma unroll
            for (int k = 0; k < 9; ++k) {
                const int dy = k % 3 - 1, dz = k / 3 - 1;
                const bool in = (uint32_t)((int)y + dy) < N && (uint32_t)((int)z + dz) < N;      // rows outside the grid are empty
                const uint64_t* p = S + (ptrdiff_t)at + ((ptrdiff_t)dz * (ptrdiff_t)N + dy) * (ptrdiff_t)W;
                const uint64_t cur = in ? p[0] : 0ull, prev = in && w ? p[-1] : 0ull, next = in && w + 1u < W ? p[1] : 0ull;
                rows[k] = thin_row(prev, cur, next);
            }
            const uint64_t now = thin_word(s, border, rows, sub & 1u, kind);
            if (now != s) {
                S[at] = now;
                gone = solid_popc(s ^ now);
            }
        }
    }
#pragma unroll
    for (uint32_t d = 1; d < 64u; d <<= 1) gone += (uint32_t)__shfl_xor((int)gone, (int)d);      // (every lane of the wave is here)
    if ((threadIdx.x & 63u) == 0u && gone) {
        (void)__hip_atomic_fetch_add(&ctl->removed, (unsigned long long)gone, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        ctl->live[iteration] = 1u;
    }
}

// One batch: (first: the pack and the copy of S,) `iterations` iterations, the write-back.  The words of the control block are cleared in front of
// the iterations; the count of removed voxels runs on from batch to batch.
hipError_t launch_thin(uint8_t* grid, uint32_t N, int kind, const ThinScratch& l, uint32_t iterations, bool first, hipStream_t s)
{
    if (!grid || !l.ctl || !l.S || !l.was || !l.B || !l.loose || N < 2u || N > kThinMaxN || (N & 1u) || (kind != THIN_CURVE && kind != THIN_KERNEL)) return hipErrorInvalidValue;
    const uint32_t W = fill_row_words(N), words = N * N * W, lanes = (N >> 1) * (N >> 1) * W;    // (N <= kThinMaxN: 2^27 words at the most)
    ThinControl* ctl = l.ctl;
    uint64_t *S = l.S, *B = l.B, *loose = l.loose;
    uint8_t* was = reinterpret_cast<uint8_t*>(l.was);
    iterations = thin_batch(iterations, 0u);
    hipError_t e = hipMemsetAsync(ctl, 0, first ? sizeof(ThinControl) : sizeof(ctl->live), s);
    if (e != hipSuccess) return e;
    if (first) {
        launch_morph_pack(grid, N, was, loose, s);
        e = hipMemcpyAsync(S, was, (size_t)words * sizeof(uint64_t), hipMemcpyDeviceToDevice, s);
        if (e != hipSuccess) return e;
    }
    const uint32_t wordBlocks = (words + 255u) / 256u, subBlocks = (lanes + 255u) / 256u;
    for (uint32_t k = 0; k < iterations; ++k) {
        k_thin_border<<<wordBlocks, 256, 0, s>>>(S, N, B, words, ctl, k);
        for (uint32_t sub = 0; sub < 8u; ++sub) k_thin_sub<<<subBlocks, 256, 0, s>>>(S, B, N, sub, kind, lanes, ctl, k);
    }
    launch_morph_write(was, reinterpret_cast<const uint8_t*>(S), loose, N, grid, ctl->written, s);
    return hipGetLastError();
}

} // namespace dxv
