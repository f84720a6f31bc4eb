// Tilted Fresnel propagator tables, written on the device (msl_set_tilt).
//   P[m] = exp(-i pi lambda dz k^2) exp(-2 pi i dz tan(theta) k),   k = f(m) / (n d),  f = the signed FFT frequency index
// along one axis of n points: the free propagation through one slice of a specimen sheared by tan(theta), a cyclic shift of
// +dz tan(theta) per slice.  The propagator stays separable, so the slice loop and the layer tap run unchanged on tables that carry
// the extra factor.  The convolution passes hold the filter of an even table only: the two filter kernels run for an axis at a zero
// tangent, and a tilt along such an axis runs on the two-pass loop (mslice.hip: set_loop_mode).  One to three launches per axis, all on
// the handle's stream, no host copy (one more, propagator_bandlimit_kernel below, under a band limit):
//
// propagator_tables_kernel: lane m forms the phase in turns in float64, t = -(lambda dz / 2 k^2 + dz tan k), reduces it to one turn
//   (t - rint(t): the reduction is exact, the phase carries the float64 rounding of its products, ~1e-15 turns; dz tan / (n d) is no
//   ratio of integers, so there is no integer form of the tilt term) and takes one float64 sincospi; every table entry is rounded once to float:
//     plain[m] = P[m] / n,   split[(m & 1) n/2 + m/2] = P[m] / n (AX_TWO),   conj[m] = conj(P[m]) (layer tap, unscaled).
//   For a convolution axis it also keeps P[m] and E[m] = exp(+2 pi i m / n) in float64 (lanes m < n) and W[l] = exp(-2 pi i l / M)
//   (lanes l < M) for the two sums below.
// conv_lag_kernel: block j < n sums a[j] = (1/n) sum_m P[m] E[(m j) mod n] -- the index reduced in integers, the products and the sum
//   in float64, a fixed tree over the block -- and places it at lags j and j - n of the length-M line q; the blocks past n zero the
//   gap [n, M - n].
// conv_filter_kernel: block e owns one stored entry of the filter: Q[k] = (1/M) sum_l q[l] W[(k l) mod M] over the 2n - 1 non-zero
//   lags, the same way; k(e) is the half-spectrum (entries 0 .. M/2, then a zero) or, for M = 4096, the even-odd layout of
//   rowTC2_pass_kernel (even k at 0 .. 1024, odd k from 1026, zeros between and behind).
// No atomics: repeated calls are bitwise equal.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace msl {

constexpr int PROP_BLOCK = 256;

// one axis: n points, kfreq = 1 / (n d), half_ldz = lambda dz / 2, shift = dz tan(theta) (Angstrom); split, Pd, Ed, Wd may be null
// (Wd is read with M > 0 only).  Lanes cover max(n, M).
__global__ void __launch_bounds__(PROP_BLOCK) propagator_tables_kernel(int n, int M, double kfreq, double half_ldz, double shift,
                                                                       float2* __restrict__ plain, float2* __restrict__ split,
                                                                       float2* __restrict__ conj, double2* __restrict__ Pd,
                                                                       double2* __restrict__ Ed, double2* __restrict__ Wd) {
    const int m = blockIdx.x * blockDim.x + threadIdx.x;
    if (m < n) {
        const double k = (double)signed_freq(m, n) * kfreq;
        double t = -fma(half_ldz * k, k, shift * k);
        t -= rint(t);
        double sn, cs;
        sincospi(2.0 * t, &sn, &cs);
        const float2 scaled = make_float2((float)(cs / n), (float)(sn / n));
        plain[m] = scaled;
        if (split) split[(m & 1) * (n / 2) + (m >> 1)] = scaled;
        conj[m] = make_float2((float)cs, (float)-sn);
        if (Pd) {
            Pd[m] = make_double2(cs, sn);
            sincospi(2.0 * ((double)m / (double)n), &sn, &cs);
            Ed[m] = make_double2(cs, sn);
        }
    }
    if (Wd && m < M) {
        double sn, cs;
        sincospi(-2.0 * ((double)m / (double)M), &sn, &cs);
        Wd[m] = make_double2(cs, sn);
    }
}

// Band limit (msl_set_bandlimit): runs after propagator_tables_kernel and before the two filter kernels, and
// zeroes the entries with |f(m)| > cut of every table of the axis -- plain, split (in its permuted order), conj and, for a convolution
// axis, the float64 copy Pd the filter sums read, so that the filter is that of the masked table.  A kept entry is not touched: with
// no entry beyond the cut the tables are bit for bit those of propagator_tables_kernel.  split and Pd may be null.
__global__ void __launch_bounds__(PROP_BLOCK) propagator_bandlimit_kernel(int n, int cut, float2* __restrict__ plain,
                                                                          float2* __restrict__ split, float2* __restrict__ conj,
                                                                          double2* __restrict__ Pd) {
    const int m = blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= n) return;
    const int f = signed_freq(m, n);
    if ((f < 0 ? -f : f) <= cut) return;
    const float2 zero = make_float2(0.f, 0.f);
    plain[m] = zero;
    if (split) split[(m & 1) * (n / 2) + (m >> 1)] = zero;
    conj[m] = zero;
    if (Pd) Pd[m] = make_double2(0.0, 0.0);
}

// sum of v over the block, in a fixed order; every lane of the block must call it
__device__ __forceinline__ double2 prop_block_sum(double2 v, double2* lds) {
    lds[threadIdx.x] = v;
    __syncthreads();
    for (int s = PROP_BLOCK / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) {
            lds[threadIdx.x].x += lds[threadIdx.x + s].x;
            lds[threadIdx.x].y += lds[threadIdx.x + s].y;
        }
        __syncthreads();
    }
    return lds[0];
}

// q: M entries (M >= 2n - 1).  grid = n + ceil((M - 2n + 1) / PROP_BLOCK) blocks
__global__ void __launch_bounds__(PROP_BLOCK) conv_lag_kernel(int n, int M, const double2* __restrict__ Pd, const double2* __restrict__ Ed,
                                                              double2* __restrict__ q) {
    __shared__ double2 lds[PROP_BLOCK];
    const int j = blockIdx.x;
    if (j >= n) {                                           // the zero gap between lag n - 1 and lag 1 - n
        const int l = n + (j - n) * PROP_BLOCK + (int)threadIdx.x;
        if (l <= M - n) q[l] = make_double2(0.0, 0.0);
        return;
    }
    double2 s = make_double2(0.0, 0.0);
    for (int m = threadIdx.x; m < n; m += PROP_BLOCK) {
        const double2 p = Pd[m], e = Ed[(int)(((long long)m * j) % n)];
        s.x += fma(p.x, e.x, -p.y * e.y);
        s.y += fma(p.x, e.y, p.y * e.x);
    }
    s = prop_block_sum(s, lds);
    if (threadIdx.x == 0) {
        const double2 a = make_double2(s.x / n, s.y / n);
        q[j] = a;
        if (j) q[M - n + j] = a;
    }
}

// qf: `entries` floats2 (conv_filter_entries); even_odd: the M = 4096 layout.  grid = entries blocks
__global__ void __launch_bounds__(PROP_BLOCK) conv_filter_kernel(int n, int M, int entries, int even_odd, const double2* __restrict__ q,
                                                                 const double2* __restrict__ Wd, float2* __restrict__ qf) {
    __shared__ double2 lds[PROP_BLOCK];
    const int e = blockIdx.x;
    if (e >= entries) return;
    int k = -1;                                             // frequency of entry e, -1: a zero entry
    if (even_odd) {
        if (e <= M / 4) k = 2 * e;
        else if (e >= M / 4 + 2 && e < M / 2 + 2) k = 2 * (e - (M / 4 + 2)) + 1;
    } else if (e <= M / 2) {
        k = e;
    }
    if (k < 0) {                                            // (uniform over the block)
        if (threadIdx.x == 0) qf[e] = make_float2(0.f, 0.f);
        return;
    }
    double2 s = make_double2(0.0, 0.0);
    for (int t = threadIdx.x; t < 2 * n - 1; t += PROP_BLOCK) {
        const int l = t < n ? t : M - 2 * n + 1 + t;        // lags 0 .. n - 1, then 1 - n .. -1 at M - n + 1 .. M - 1
        const double2 a = q[l], w = Wd[(int)(((long long)k * l) & (M - 1))];
        s.x += fma(a.x, w.x, -a.y * w.y);
        s.y += fma(a.x, w.y, a.y * w.x);
    }
    s = prop_block_sum(s, lds);
    if (threadIdx.x == 0) qf[e] = make_float2((float)(s.x / M), (float)(s.y / M));
}

}  // namespace msl
