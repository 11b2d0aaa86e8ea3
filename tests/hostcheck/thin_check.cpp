// The product's thinning routines (csrc/dxv_thin.h) compiled for the CPU: the same chain as csrc/thin.hip -- pack, per iteration the border and
// the eight sub-iterations over the words of a quarter of the rows, write-back -- with a loop where the device has a grid of threads.  A
// sub-iteration works in place here too: the bits a word's decision looks at belong to other subfields than the ones it may clear.
// tests/thin_host.py loads this; tests/test_thin_rule.py compares it with the numpy restatement.
#include <stdint.h>
#include <string.h>
#include <vector>
#include "../../dxrvoxelizer_amd/csrc/dxv_morph.h"
#include "../../dxrvoxelizer_amd/csrc/dxv_thin.h"

using namespace dxv;

static uint64_t word_at(const std::vector<uint64_t>& S, uint32_t N, uint32_t W, int64_t y, int64_t z, int64_t w)
{
    if (y < 0 || z < 0 || w < 0 || y >= (int64_t)N || z >= (int64_t)N || w >= (int64_t)W) return 0ull;
    return S[((size_t)z * N + (size_t)y) * W + (size_t)w];
}

extern "C" {

// grid: N^3 bytes, thinned in place; eight: the 8-byte path of pack and write-back where N % 8 == 0; out: {iterations, removed, converged}
int tc_thin(uint8_t* grid, uint32_t N, int kind, uint32_t maxIterations, int eight, uint64_t* out)
{
    if (N < 2u || N > kThinMaxN || (N & 1u) || (kind != THIN_CURVE && kind != THIN_KERNEL)) return 1;
    const uint32_t W = fill_row_words(N), rowBytes = W * 8u;
    const size_t words = (size_t)N * N * W, bytes = words * 8u;
    const bool wide = eight && (N & 7u) == 0u;
    std::vector<uint64_t> was(words), S, B(words);
    std::vector<uint8_t> loose(bytes);
    uint8_t* pk = reinterpret_cast<uint8_t*>(was.data());
    for (size_t t = 0; t < bytes; ++t) {
        const size_t row = t / rowBytes;
        const uint32_t j = (uint32_t)(t % rowBytes);
        uint32_t bits = 0;
        bool odd = false;
        if (8u * j < N) {
            const uint8_t* g = grid + row * N;
            if (wide) {
                uint64_t e;
                memcpy(&e, g + 8u * j, 8);
                bits = morph_member_byte(e, false); odd = morph_loose(e);
            }
            else { bits = morph_member_byte(g, N, j, false); odd = morph_loose(g, N, j); }
        }
        pk[t] = (uint8_t)bits;
        loose[t] = odd;
    }
    S = was;
    uint64_t iterations = 0, removed = 0;
    bool converged = false;
    while (!maxIterations || iterations < maxIterations) {
        ++iterations;
        for (size_t t = 0; t < words; ++t) {
            const int64_t w = (int64_t)(t % W), row = (int64_t)(t / W), y = row % N, z = row / N;
            B[t] = thin_border_word(S[t], word_at(S, N, W, y, z, w - 1), word_at(S, N, W, y, z, w + 1), word_at(S, N, W, y - 1, z, w), word_at(S, N, W, y + 1, z, w),
                                    word_at(S, N, W, y, z - 1, w), word_at(S, N, W, y, z + 1, w));
        }
        uint64_t gone = 0;
        for (uint32_t sub = 0; sub < 8u; ++sub)
            for (uint32_t z = (sub >> 2) & 1u; z < N; z += 2u)
                for (uint32_t y = (sub >> 1) & 1u; y < N; y += 2u)
                    for (uint32_t w = 0; w < W; ++w) {
                        const size_t at = ((size_t)z * N + y) * W + w;
                        const uint64_t s = S[at];
                        if (!(s & B[at] & thin_x_parity(sub & 1u))) continue;
                        ThinRow rows[9];
                        for (int k = 0; k < 9; ++k) {
                            const int64_t yy = (int64_t)y + k % 3 - 1, zz = (int64_t)z + k / 3 - 1;
                            rows[k] = thin_row(word_at(S, N, W, yy, zz, (int64_t)w - 1), word_at(S, N, W, yy, zz, w), word_at(S, N, W, yy, zz, (int64_t)w + 1));
                        }
                        const uint64_t now = thin_word(s, B[at], rows, sub & 1u, kind);
                        gone += solid_popc(s ^ now);
                        S[at] = now;
                    }
        removed += gone;
        if (!gone) { converged = true; break; }
    }
    const uint8_t* now = reinterpret_cast<const uint8_t*>(S.data());
    for (size_t t = 0; t < bytes; ++t) {
        const size_t row = t / rowBytes;
        const uint32_t j = (uint32_t)(t % rowBytes);
        if (8u * j >= N) continue;
        const uint32_t left = N - 8u * j, valid = left >= 8u ? 0xffu : (1u << left) - 1u;
        const uint32_t before = pk[t] & valid, after = now[t] & valid;
        if (before == after && !loose[t]) continue;
        uint8_t* g = grid + row * N + 8u * j;
        if (wide) { const uint64_t e = fill_spread_byte(after); memcpy(g, &e, 8); }
        else
            for (uint32_t k = 0; k < 8u && k < left; ++k) g[k] = (uint8_t)((after >> k) & 1u);
    }
    if (out) { out[0] = iterations; out[1] = removed; out[2] = converged ? 1u : 0u; }
    return 0;
}

uint32_t tc_T26(uint32_t cfg) { return thin_T26(cfg); }
uint32_t tc_T6(uint32_t cfg) { return thin_T6(cfg); }
int tc_simple(uint32_t cfg) { return thin_simple(cfg) ? 1 : 0; }
int tc_keeps(int kind, uint32_t cfg) { return thin_keeps(kind, cfg) ? 1 : 0; }
// many at once: bit 0 simple, bit 1 kept by CURVE, bits 8.. T26, bits 16.. T6
void tc_decide(const uint32_t* cfg, size_t count, uint32_t* out)
{
    for (size_t i = 0; i < count; ++i)
        out[i] = (thin_simple(cfg[i]) ? 1u : 0u) | (thin_keeps(THIN_CURVE, cfg[i]) ? 2u : 0u) | (thin_T26(cfg[i]) << 8) | (thin_T6(cfg[i]) << 16);
}
uint32_t tc_three(uint64_t prev, uint64_t cur, uint64_t next, uint32_t b) { return thin_three(thin_row(prev, cur, next), b); }
uint32_t tc_batch(uint32_t rounds, uint32_t left) { return thin_batch(rounds, left); }
uint32_t tc_rounds_default(void) { return kThinRoundsDefault; }
uint32_t tc_rounds_max(void) { return kThinMaxRounds; }
uint32_t tc_max_n(void) { return kThinMaxN; }

}
