// The product's flood-fill routines (dxrvoxelizer_amd/csrc/dxv_fill.h) compiled for the CPU: the same text the kernels of fill.hip run,
// driven here in the kernels' order -- pack, then rounds of rows along x, columns along y, columns along z until one changes nothing,
// then the write-back.  Also what the option table (dxv_policy.h) says about the fill's one key.
#include "../../dxrvoxelizer_amd/csrc/dxv_fill.h"
#include "../../dxrvoxelizer_amd/csrc/dxv_policy.h"

#include <string.h>
#include <vector>

using namespace dxv;

// grid: N^3 bytes in, the filled grid out (what = 0 / 1); *rounds: rounds taken, the confirming one included.  eightAtOnce != 0: the
// pack and the write-back take the 8-byte path where the kernels take it (N % 8 == 0), else the byte path everywhere.
extern "C" int fc_fill(uint8_t* grid, uint32_t N, int what, int eightAtOnce, uint32_t* rounds)
{
    if (N < 2 || N > 2048 || (what != 0 && what != 1)) return 1;
    const uint32_t W = fill_row_words(N), rowBytes = W * 8u;
    const size_t rows = (size_t)N * N, words = fill_mask_words(N);
    std::vector<uint64_t> freeMask(words), reached(words);
    uint8_t* fb = reinterpret_cast<uint8_t*>(freeMask.data());
    uint8_t* rb = reinterpret_cast<uint8_t*>(reached.data());
    const bool eight = eightAtOnce && (N & 7u) == 0u;
#pragma omp parallel for
    for (long long row = 0; row < (long long)rows; ++row)
        for (uint32_t j = 0; j < rowBytes; ++j) {
            uint32_t free8 = 0;
            const uint8_t* g = grid + (size_t)row * N;
            if (8u * j < N) {
                if (eight) {
                    uint64_t v;
                    memcpy(&v, g + 8u * j, 8);
                    free8 = fill_free_byte(v);
                } else free8 = fill_free_byte(g, N, j);
            }
            fb[(size_t)row * rowBytes + j] = (uint8_t)free8;
            rb[(size_t)row * rowBytes + j] = (uint8_t)fill_seed_byte(free8, N, j, (uint32_t)(row % N), (uint32_t)(row / N));
        }
    uint32_t done = 0;
    for (;;) {
        int changed = 0;
#pragma omp parallel for reduction(| : changed)
        for (long long row = 0; row < (long long)rows; ++row) changed |= fill_row(freeMask.data() + (size_t)row * W, reached.data() + (size_t)row * W, W) ? 1 : 0;
        const uint32_t columns = N * W;
#pragma omp parallel for reduction(| : changed)
        for (long long i = 0; i < (long long)columns; ++i) {             // i = iz * W + w
            const size_t base = (size_t)(i / W) * N * W + (size_t)(i % W);
            FillColumn col{freeMask.data() + base, reached.data() + base, W, N};
            changed |= col.run() ? 1 : 0;
        }
#pragma omp parallel for reduction(| : changed)
        for (long long i = 0; i < (long long)columns; ++i) {             // i = iy * W + w
            FillColumn col{freeMask.data() + i, reached.data() + i, (size_t)N * W, N};
            changed |= col.run() ? 1 : 0;
        }
        ++done;
        if (!changed) break;
        if (done > (uint32_t)(N * N) * N) return 2;
    }
    if (rounds) *rounds = done;
#pragma omp parallel for
    for (long long row = 0; row < (long long)rows; ++row)
        for (uint32_t j = 0; 8u * j < N; ++j) {
            const uint32_t bits = fill_result_byte(fb[(size_t)row * rowBytes + j], rb[(size_t)row * rowBytes + j], what);
            uint8_t* g = grid + (size_t)row * N + 8u * j;
            if (eight) {
                const uint64_t v = fill_spread_byte(bits);
                memcpy(g, &v, 8);
            } else
                for (uint32_t k = 0; k < 8u && 8u * j + k < N; ++k) g[k] = (uint8_t)((bits >> k) & 1u);
        }
    return 0;
}

// the word routines on their own: every run of f that holds a bit of r
extern "C" uint64_t fc_fill_word(uint64_t r, uint64_t f) { return fill_word(r, f); }

// dxv_set_option's view of a key: -1 unknown, else 1 / 0 = the value is accepted / refused; and the key's default
extern "C" int fc_option_accepts(const char* name, int64_t value)
{
    const OptionRow* row = find_option(name);
    return row ? (option_accepts(row->rule, value) ? 1 : 0) : -1;
}
extern "C" int fc_option_default(const char* name)
{
    const OptionRow* row = find_option(name);
    const Options defaults;
    return row ? defaults.*row->where : -1;
}
extern "C" int fc_default_rounds(void) { return (int)kFillRoundsDefault; }
