// Finite dose (msl_dose_reset / msl_dose_add / msl_dose_counts, include/mslice.h): Poisson counts of the frame-summed patterns of a
// probe batch, drawn where the patterns are.  The definition is pyslice_amd/dose.py (poisson_counts):
//   counter of pixel i (row-major in the (mx, my) pattern), probe p, attempt t: (i, p, t, 0)     key: (seed & 0xffffffff, seed >> 32)
//   x0..x3 = Philox-4x32-10 (thermal.h)      U(hi, lo) = (((hi >> 6) << 26 | (lo >> 6)) + 0.5) 2^-52     u = U(x0, x1), v = U(x2, x3)
//   lam == 0: 0, nothing drawn
//   lam < 10: inversion by sequential search on attempt 0, at most DOSE_K_LIMIT steps
//   lam >= 10: Hoermann's PTRS, one block per attempt, at most DOSE_ATTEMPTS, then rint(lam)
//   counts saturate at 2^32 - 1
// The accumulator is filled by diffract_kernel<.., ACC = true> (diffract.h): the frame sums of every msl_dose_add are added in call order.
// dose_counts_kernel: one thread per pixel of (B, mx my); lam = acc * scale is ONE float64 multiply and no product is fused into a
// sum below (fp contract off), so that the host reproduces every comparison from the float64 it is given -- up to the last place of
// exp / log / lgamma.  The rejection loop diverges per lane; both loops have fixed bounds.  A negative or non-finite lam writes 1 to
// the flag word (a plain vector store; every lane that finds one stores the same value) and a count of 0.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "thermal.h"

namespace msl {

constexpr int DOSE_K_LIMIT = 96;        // inversion: the largest count of lam < 10
constexpr int DOSE_ATTEMPTS = 64;       // PTRS: attempts before rint(lam)

__device__ __forceinline__ double dose_uniform(uint32_t hi, uint32_t lo) {
    const uint64_t m = ((uint64_t)(hi >> 6) << 26) | (uint64_t)(lo >> 6);      // 52 bits: m + 0.5 is exact
    return ((double)m + 0.5) * 0x1p-52;
}

__device__ __forceinline__ uint32_t dose_saturate(double k) {
    return k >= 4294967295.0 ? 0xffffffffu : (k > 0.0 ? (uint32_t)k : 0u);
}

__device__ inline uint32_t dose_poisson(double lam, uint32_t pixel, uint32_t probe, uint32_t k0, uint32_t k1) {
#pragma clang fp contract(off)
    if (lam == 0.0) return 0u;
    if (lam < 10.0) {
        uint32_t x[4] = {pixel, probe, 0u, 0u};
        philox4x32_10(x, k0, k1);
        const double u = dose_uniform(x[0], x[1]);
        double p = exp(-lam), s = p;
        int k = 0;
        while (u > s && k < DOSE_K_LIMIT) {
            ++k;
            p *= lam / (double)k;
            s += p;
        }
        return (uint32_t)k;
    }
    const double slam = sqrt(lam), loglam = log(lam);
    const double b = 0.931 + 2.53 * slam;
    const double a = -0.059 + 0.02483 * b;
    const double invalpha = 1.1239 + 1.1328 / (b - 3.4);
    const double vr = 0.9277 - 3.6224 / (b - 2.0);
    for (uint32_t attempt = 0; attempt < (uint32_t)DOSE_ATTEMPTS; ++attempt) {
        uint32_t x[4] = {pixel, probe, attempt, 0u};
        philox4x32_10(x, k0, k1);
        const double u = dose_uniform(x[0], x[1]), v = dose_uniform(x[2], x[3]);
        const double U = u - 0.5;
        const double us = 0.5 - fabs(U);
        const double k = floor((2.0 * a / us + b) * U + lam + 0.43);
        if (us >= 0.07 && v <= vr) return dose_saturate(k);
        if (k < 0.0 || (us < 0.013 && v > us)) continue;
        const double lhs = log(v) + log(invalpha) - log(a / (us * us) + b);
        const double rhs = -lam + k * loglam - lgamma(k + 1.0);
        if (lhs <= rhs) return dose_saturate(k);
    }
    return dose_saturate(rint(lam));
}

// counts[idx] of pixel idx = b * K + i of the accumulator (B, K): the draw of lam = acc[idx] * scale for probe probe0 + b
__global__ void __launch_bounds__(256) dose_counts_kernel(const double* __restrict__ acc, long long n, long long K, double scale, uint32_t k0,
                                                          uint32_t k1, uint32_t probe0, uint32_t* __restrict__ counts,
                                                          uint32_t* __restrict__ flag) {
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= n) return;
    const long long b = idx / K;
    const double lam = acc[idx] * scale;
    if (!(lam >= 0.0) || lam > 1.7976931348623157e308) {        // negative, NaN or infinite
        *flag = 1u;
        counts[idx] = 0u;
        return;
    }
    counts[idx] = dose_poisson(lam, (uint32_t)(idx - b * K), probe0 + (uint32_t)b, k0, k1);
}

}  // namespace msl
