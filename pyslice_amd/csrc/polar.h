// Polar detector pass (msl_polar_detect): the intensity of every exit spectrum summed into R radial rings x A azimuthal sectors.
//   out[row, b] = sum over the pixels k of bin b of |Psi[row, k]|^2,   bin[k] = r * A + a, or POLAR_NONE for a pixel in no bin.
// Rows of K stored pixels start every `ld` pixels; row r = b * count + j is frame slot t0 + j of probe b of a (B, T, ld) array.
//
// Bin-sorted gather.  polar_layout() (host, no device) sorts the pixels by bin once, stably: `order` lists the pixel indices of
// bin 0 ascending, then bin 1 ...; seg[b] .. seg[b + 1] is bin b's slice of it.  One wave owns one bin for a block of rows: lane l
// reads order[seg[b] + l], + 64, ... (coalesced, one step ahead), gathers Psi[row][order[i]] of POLAR_ROWS rows at a time (independent 8-byte
// loads), forms |Psi|^2 in fp32 and adds it into a float64 accumulator per row; the wave ends with the fixed xor tree 32, 16, .., 1
// on float64 and lane 0 stores out[row][b].  No partial slab, no finishing kernel, no atomics: the summation order is fixed by
// (order, seg) alone, so the same input gives bitwise the same output.  An empty bin stores exactly 0.
// The grid is walked row-major: consecutive workgroups take the bin groups of one row block, so the gathered cache lines of a row
// (2 MB at 512 x 512) are shared through L2 by the bins that touch them.  Only indices below K are ever in `order`: the pad pixels
// K <= k < ld are never read.
#pragma once
#include <stdint.h>

#include <vector>

namespace msl {

constexpr uint16_t POLAR_NONE = 0xFFFF;        // include/mslice.h: MSL_POLAR_NONE
constexpr int POLAR_MAX_BINS = 4096;            // include/mslice.h: MSL_POLAR_MAX_BINS
constexpr int POLAR_ROWS = 4;                   // rows a wave gathers together: loads in flight per lane
constexpr int POLAR_WAVES = 4;                  // bins per workgroup

// Stable counting sort of the K pixels by bin: order[seg[b] .. seg[b + 1]) = the pixels of bin b, ascending; seg has n_bins + 1
// entries, seg[n_bins] = the pixels in any bin (order has room for K).  false: a bin id >= n_bins that is not POLAR_NONE.
inline bool polar_layout(const uint16_t* bin, int64_t K, int32_t n_bins, uint32_t* order, int64_t* seg) {
    std::vector<int64_t> fill((size_t)n_bins + 1, 0);
    for (int64_t k = 0; k < K; ++k) {
        const uint16_t b = bin[k];
        if (b == POLAR_NONE) continue;
        if ((int32_t)b >= n_bins) return false;
        ++fill[(size_t)b + 1];
    }
    for (int32_t b = 0; b < n_bins; ++b) fill[(size_t)b + 1] += fill[b];
    for (int32_t b = 0; b <= n_bins; ++b) seg[b] = fill[b];
    for (int64_t k = 0; k < K; ++k) {
        const uint16_t b = bin[k];
        if (b != POLAR_NONE) order[fill[b]++] = (uint32_t)k;
    }
    return true;
}

}  // namespace msl

#ifdef __HIPCC__
#include <hip/hip_runtime.h>

namespace msl {

// workgroup w of the linear grid: row block w / bin_groups, bins (w % bin_groups) * POLAR_WAVES + wave
__global__ void __launch_bounds__(64 * POLAR_WAVES) polar_gather_kernel(const float2* __restrict__ src, long long T, long long t0, unsigned count,
                                                                        long long ld, long long rows, int rows_per_wg, int n_bins,
                                                                        unsigned bin_groups, const uint32_t* __restrict__ order,
                                                                        const long long* __restrict__ seg, double* __restrict__ out) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned rb = blockIdx.x / bin_groups;                  // (rows < 2^31: row and workgroup indices divide as 32-bit numbers)
    const long long b = (long long)(blockIdx.x - rb * bin_groups) * POLAR_WAVES + wave;
    if (b >= n_bins) return;                                      // (wave-uniform: no barrier in this kernel)
    const long long s0 = seg[b], s1 = seg[b + 1];
    const long long r0 = (long long)rb * rows_per_wg;
    const long long r1 = min(rows, r0 + rows_per_wg);
    for (long long r = r0; r < r1; r += POLAR_ROWS) {
        // rows past the block's end repeat its last row (their sums are not stored): no branch around the loads
        const float2* row[POLAR_ROWS];
#pragma unroll
        for (int u = 0; u < POLAR_ROWS; ++u) {
            const unsigned rr = (unsigned)min(r + u, r1 - 1);
            const unsigned p = rr / count, j = rr - p * count;
            row[u] = src + ((long long)p * T + t0 + j) * ld;
        }
        double acc[POLAR_ROWS];
#pragma unroll
        for (int u = 0; u < POLAR_ROWS; ++u) acc[u] = 0.0;
        // the index of the next step is loaded with the gathers of this one: one memory latency per step, not two
        long long i = s0 + lane;
        uint32_t k = i < s1 ? order[i] : 0u;
        while (i < s1) {
            const long long in = i + 64;
            const uint32_t kn = in < s1 ? order[in] : 0u;
            float2 z[POLAR_ROWS];
#pragma unroll
            for (int u = 0; u < POLAR_ROWS; ++u) z[u] = row[u][k];
#pragma unroll
            for (int u = 0; u < POLAR_ROWS; ++u) acc[u] += (double)(z[u].x * z[u].x + z[u].y * z[u].y);
            i = in;
            k = kn;
        }
#pragma unroll
        for (int u = 0; u < POLAR_ROWS; ++u) {
            double v = acc[u];
#pragma unroll
            for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
            if (lane == 0 && r + u < r1) out[(r + u) * n_bins + b] = v;
        }
    }
}

}  // namespace msl
#endif
