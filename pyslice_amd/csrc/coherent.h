// Coherent accumulation pass (msl_coherent_add / msl_coherent_finish): the per-pixel complex sum of the frames of every probe, for the
// elastic part |<Psi>|^2 of a frozen-phonon run.
//   acc[b, k] += sum_{j < count} Psi[b, t0 + j, k]       k < K, over a (B, T, K) complex64 array whose images start every `ld` pixels;
//   out[(b * mx + ix) * my + iy] = sum_{a < bx} sum_{c < by} |acc[b, (ix * bx + a) * wy + iy * by + c]|^2 / n^2.
// acc is (B, pitch) double2 (re, im), owned by the handle.
//
// coherent_add_kernel is pixel-major: a lane owns one column pair of one image (16-byte loads of Psi, 32 bytes of accumulator read
// and written once per launch; one column with 8-byte loads when ld, K or the base address is odd) and walks the `count` frames
// COH_ROWS at a time: the loads of a batch are independent (their frame offsets are wave-uniform).  Every addend is widened to
// float64 BEFORE it is added: the pass is bound by HBM, not by float64 adds, and a coherent sum is all cancellation -- the Bragg
// amplitudes of T frames add up, the thermal part nearly cancels.  The frames are added in order onto the value the accumulator
// holds, so one call over [0, T) and calls over [0, s) and [s, T) perform the same additions.  No atomics: repeated sequences are
// bitwise equal.  Pad pixels (K <= k < ld) are never read.
// coherent_finish_kernel runs once per probe batch and has no speed target: L lanes (a power of two <= 64) share a bin, each adds
// every L-th pixel of it in float64, an xor exchange adds the L partial sums in a fixed order, the bin's first lane stores.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>

namespace msl {

constexpr int COH_ROWS = 8;                     // frames in flight per lane (tail: 4, 2, 1)

template <bool VEC>
__global__ void __launch_bounds__(256) coherent_add_kernel(const float2* __restrict__ src, long long B, long long T, long long t0, int count,
                                                           long long ld, long long K, long long pitch, double2* __restrict__ acc) {
    constexpr int PXL = VEC ? 2 : 1;            // columns per lane
    const long long k = ((long long)blockIdx.x * blockDim.x + threadIdx.x) * PXL;
    if (k >= K) return;                         // VEC: K is even, so k + 1 < K as well
    for (long long b = blockIdx.y; b < B; b += gridDim.y) {
        const float2* base = src + (b * T + t0) * ld + k;
        double2* a = acc + b * pitch + k;
        double2 s0 = a[0], s1 = make_double2(0.0, 0.0);
        if constexpr (VEC) s1 = a[1];
        long long off = 0;                      // wave-uniform: offset of frame t0 + j
        // N frames: N independent loads, then the N values widened and added in frame order
        auto batch = [&](auto n_tag) {
            constexpr int N = decltype(n_tag)::value;
            if constexpr (VEC) {
                float4 v[N];
#pragma unroll
                for (int u = 0; u < N; ++u) v[u] = *reinterpret_cast<const float4*>(base + off + u * ld);
#pragma unroll
                for (int u = 0; u < N; ++u) {
                    s0.x += (double)v[u].x; s0.y += (double)v[u].y;
                    s1.x += (double)v[u].z; s1.y += (double)v[u].w;
                }
            } else {
                float2 v[N];
#pragma unroll
                for (int u = 0; u < N; ++u) v[u] = base[off + u * ld];
#pragma unroll
                for (int u = 0; u < N; ++u) { s0.x += (double)v[u].x; s0.y += (double)v[u].y; }
            }
            off += N * ld;
        };
        int j = 0;
        for (; j + COH_ROWS <= count; j += COH_ROWS) batch(std::integral_constant<int, COH_ROWS>{});
        if ((count - j) & 4) batch(std::integral_constant<int, 4>{});
        if ((count - j) & 2) batch(std::integral_constant<int, 2>{});
        if ((count - j) & 1) batch(std::integral_constant<int, 1>{});
        a[0] = s0;
        if constexpr (VEC) a[1] = s1;
    }
}

// bins = B * mx * my; thread g serves bin g / L as its lane g % L (L divides the wave, so the lanes of a bin sit in one wave)
__global__ void __launch_bounds__(256) coherent_finish_kernel(const double2* __restrict__ acc, long long pitch, long long bins, int wy, int mx, int my,
                                                              int bx, int by, int L, double n2, double* __restrict__ out) {
    const long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long bin = g / L;
    const int l = (int)(g - bin * L);
    double v = 0.0;
    const bool live = bin < bins;               // (the dead lanes of the last wave still take part in the exchange)
    if (live) {
        const long long b = bin / ((long long)mx * my);
        const int r = (int)(bin - b * mx * my);
        const int ix = r / my, iy = r - ix * my;
        const double2* p = acc + b * pitch + (long long)ix * bx * wy + (long long)iy * by;
        const int n = bx * by;
        for (int i = l; i < n; i += L) {
            const int a = i / by, c = i - a * by;
            const double2 z = p[(long long)a * wy + c];
            v += z.x * z.x + z.y * z.y;
        }
    }
    for (int o = L >> 1; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
    if (live && l == 0) out[bin] = v / n2;
}

}  // namespace msl
