// measure.hip -- the integral measures of the components of a labelling (dxv_measure.h has the rule's word routines), on the frame's stream.  One
// pass over the member mask; the grid, the labels and the component table are read, never written:
//   (memset)           the K + 1 records to zero
//   k_measure<6 | 26>  one lane per mask word, a step of the wave's loop per run of the lane's word (the walk of k_comp_stats): the word's
//                      neighbour rows once (six rows at 6, nine at 26, three words each), then per run one load of a label and the twelve
//                      values of meas_run.  The runs a wave holds in a step that have the label of its first one -- all of them, when the
//                      wave holds one label -- are added up with shuffles and one lane sends the total; a run with another label is sent
//                      by its own lane (a wave that one small component passes through does not fall back to 64 sends to the large one
//                      round it: DESIGN §4.13 has the times of both).  A send is a 64-bit agent-scope relaxed
//                      fetch_add per value into the component's record (euler by two's complement), served by the L2 all CUs share; a value
//                      of 0 is not sent.  Sums only: no arrival order shows.
//   k_measure_total    one lane per record 1 .. K: the wave adds its records up and one lane adds them to record 0.
// There is no second level of aggregation (a workgroup gathering its leading label in LDS): DESIGN §4.13 has what was measured.
// Every loop ends because bits leave a word.  No kernel waits for another workgroup, none uses scratch memory or LDS.
#include "dxv_device.h"
#include "dxv_measure.h"

namespace dxv {

__device__ __forceinline__ void measure_send(unsigned long long* record, const uint64_t* v)
{
#pragma unroll
    for (uint32_t k = 0; k < kMeasureValues; ++k)
        if (v[k]) (void)__hip_atomic_fetch_add(record + k, (unsigned long long)v[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// every lane of the wave is here
__device__ __forceinline__ void measure_wave_sum(uint64_t* v)
{
#pragma unroll
    for (uint32_t k = 0; k < kMeasureValues; ++k) {
        unsigned long long x = v[k];
#pragma unroll
        for (uint32_t d = 1; d < 64u; d <<= 1) x += __shfl_xor(x, (int)d);
        v[k] = x;
    }
}

// table: (K + 1) * kMeasureValues 64-bit words, zero
template <uint32_t kConn>
__global__ __launch_bounds__(256) void k_measure(const uint64_t* __restrict__ mask, uint32_t N, const uint32_t* __restrict__ labels, unsigned long long* table,
                                                 uint32_t words, uint32_t K)
{
    const uint32_t t = blockIdx.x * 256u + threadIdx.x, lane = threadIdx.x & 63u;
    const uint32_t W = fill_row_words(N);
    uint64_t m = 0;
    uint32_t row = 0, w = 0;
    if (t < words) { row = t / W; w = t - row * W; m = mask[t]; }
    const uint32_t y = row % N, z = row / N, base = row * N + 64u * w;
    MeasWord<kConn> cells = {};
    if (m) {
        MeasRow rows[9];
        meas_load_rows(mask, N, kConn, y, z, w, rows);
        meas_word<kConn>(rows, cells);
    }
    while (__any(m != 0ull)) {
        uint32_t label = 0, len = 0, s = 0;
        if (m) {
            comp_take_run(m, s, len);
            label = labels[base + s];
            if (label == 0u || label > K) len = 0u;                     // (never: a member has a label 1 .. K; no index leaves the table)
        }
        const uint64_t act = __ballot(len != 0u);
        if (!act) continue;
        const uint32_t lead = comp_ctz(act);
        const uint32_t firstLabel = (uint32_t)__shfl((int)label, (int)lead);
        uint64_t v[kMeasureValues] = {};                                // nothing for a lane without a run
        if (len) meas_run<kConn>(cells, s, len, 64u * w + s, y, z, v);
        // the runs with the label of the wave's first one -- all of them, when the wave holds one label -- are added up in registers and
        // one lane sends the total; a run with another label is sent by its own lane
        const bool own = len != 0u && label != firstLabel;
        if (own) measure_send(table + (size_t)label * kMeasureValues, v);
        if (own) {
#pragma unroll
            for (uint32_t k = 0; k < kMeasureValues; ++k) v[k] = 0ull;
        }
        measure_wave_sum(v);                                            // (every lane of the wave is here)
        if (lane == lead) measure_send(table + (size_t)firstLabel * kMeasureValues, v);
    }
}

__global__ __launch_bounds__(256) void k_measure_total(unsigned long long* table, uint32_t K)
{
    const uint32_t k = blockIdx.x * 256u + threadIdx.x, lane = threadIdx.x & 63u;
    uint64_t v[kMeasureValues] = {};
    if (k < K) {
#pragma unroll
        for (uint32_t i = 0; i < kMeasureValues; ++i) v[i] = table[((size_t)k + 1u) * kMeasureValues + i];
    }
    measure_wave_sum(v);                                                // (every lane of the wave is here)
    if (lane == 0u) measure_send(table, v);
}

size_t measure_table_bytes(uint32_t K) { return ((size_t)K + 1u) * sizeof(MeasureRecord); }

// the table of the K components whose labels stand in `labels` and whose members in `mask` (the labelling's own, or packed again from the grid)
hipError_t launch_measure(const uint64_t* mask, uint32_t N, uint32_t connectivity, const uint32_t* labels, uint32_t K, uint8_t* table, hipStream_t s)
{
    if (N < 2u || N > kCompMaxN || (N & 1u) || (connectivity != 6u && connectivity != 26u) || !mask || !labels || !table) return hipErrorInvalidValue;
    const hipError_t e = hipMemsetAsync(table, 0, measure_table_bytes(K), s);
    if (e != hipSuccess) return e;
    if (!K) return hipSuccess;
    const uint32_t maskWords = N * N * fill_row_words(N);
    unsigned long long* t = reinterpret_cast<unsigned long long*>(table);
    if (connectivity == 26u) k_measure<26u><<<(maskWords + 255u) / 256u, 256, 0, s>>>(mask, N, labels, t, maskWords, K);
    else k_measure<6u><<<(maskWords + 255u) / 256u, 256, 0, s>>>(mask, N, labels, t, maskWords, K);
    k_measure_total<<<(K + 255u) / 256u, 256, 0, s>>>(t, K);
    return hipGetLastError();
}

} // namespace dxv
