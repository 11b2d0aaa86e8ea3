// The product's measure routines (csrc/dxv_measure.h) compiled for the CPU: the same chain as csrc/measure.hip -- the member mask packed from the
// grid, every mask word's neighbour rows, every run of the word, the run's twelve values added to the record of its label -- with a loop where
// the device has a grid of threads and plain additions where it has atomics.  tests/measure_host.py loads this; tests/test_measure_rule.py
// compares it with the numpy restatement.
#include <stdint.h>
#include <string.h>
#include <vector>
#include "../../dxrvoxelizer_amd/csrc/dxv_measure.h"

using namespace dxv;

template <uint32_t kConn> static int walk(const std::vector<uint64_t>& mask, uint32_t N, const uint32_t* labels, uint32_t K, uint64_t* table)
{
    const uint32_t W = fill_row_words(N);
    for (uint32_t z = 0; z < N; ++z)
        for (uint32_t y = 0; y < N; ++y)
            for (uint32_t w = 0; w < W; ++w) {
                uint64_t m = mask[((size_t)z * N + y) * W + w];
                if (!m) continue;
                MeasRow rows[9];
                MeasWord<kConn> cells;
                meas_load_rows(mask.data(), N, kConn, y, z, w, rows);
                meas_word<kConn>(rows, cells);
                while (m) {
                    uint32_t s, len;
                    comp_take_run(m, s, len);
                    const uint32_t x0 = 64u * w + s;
                    const uint32_t label = labels[((size_t)z * N + y) * N + x0];
                    if (label == 0u || label > K) return 2;             // the labels are not a labelling of this mask
                    for (uint32_t i = 1; i < len; ++i)
                        if (labels[((size_t)z * N + y) * N + x0 + i] != label) return 3;   // (a run has one label)
                    uint64_t v[kMeasureValues];
                    meas_run<kConn>(cells, s, len, x0, y, z, v);
                    for (uint32_t i = 0; i < kMeasureValues; ++i) {
                        table[(size_t)label * kMeasureValues + i] += v[i];
                        table[i] += v[i];
                    }
                }
            }
    return 0;
}

extern "C" {

// grid: N^3 bytes; labels: N^3 uint32 of a labelling of kind `of` with K components; table: (K + 1) * 96 bytes, written
int mc_measure(const uint8_t* grid, uint32_t N, int of, uint32_t connectivity, const uint32_t* labels, uint32_t K, uint64_t* table)
{
    if (N < 2u || N > kCompMaxN || (N & 1u) || (of != COMP_SOLID && of != COMP_EMPTY) || (connectivity != 6u && connectivity != 26u)) return 1;
    const uint32_t W = fill_row_words(N), rowBytes = W * 8u;
    std::vector<uint64_t> mask((size_t)N * N * W);
    uint8_t* bytes = reinterpret_cast<uint8_t*>(mask.data());
    for (size_t t = 0; t < mask.size() * 8u; ++t) {
        const size_t row = t / rowBytes;
        const uint32_t j = (uint32_t)(t % rowBytes);
        bytes[t] = 8u * j < N ? (uint8_t)comp_member_byte(grid + row * N, N, j, of) : 0u;
    }
    memset(table, 0, ((size_t)K + 1u) * sizeof(MeasureRecord));
    return connectivity == 26u ? walk<26u>(mask, N, labels, K, table) : walk<6u>(mask, N, labels, K, table);
}

// one run by itself: the word `cur` of a row of its own (every other row clear), bits s .. s + len - 1 at x0, y, z
void mc_run(uint64_t prev, uint64_t cur, uint64_t next, uint32_t connectivity, uint32_t s, uint32_t len, uint32_t x0, uint32_t y, uint32_t z, uint64_t* v)
{
    MeasRow rows[9];
    for (int k = 0; k < 9; ++k) rows[k] = MeasRow{0ull, 0ull, 0ull};
    rows[4] = meas_row(prev, cur, next);
    if (connectivity == 26u) { MeasWord<26u> c; meas_word<26u>(rows, c); meas_run<26u>(c, s, len, x0, y, z, v); }
    else { MeasWord<6u> c; meas_word<6u>(rows, c); meas_run<6u>(c, s, len, x0, y, z, v); }
}

uint32_t mc_record_bytes(void) { return (uint32_t)sizeof(MeasureRecord); }
uint32_t mc_max_n(void) { return kCompMaxN; }

}
