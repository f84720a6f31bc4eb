// Absorptive potential: the thermally averaged transmission function of one pass,
//     t_s = exp(i sigma Vbar_s - sigma^2 Omega_s),
// Vbar the Debye-Waller-smeared mean potential and Omega = 1/2 Var V under the Gaussian displacement of every atom (the second
// cumulant of <exp(i sigma V)>: Hall-Hirsch absorption of atoms projected into one slice).  Both superpose linearly over independent
// atoms, so both are the structure-factor sum of the potential build with other per-species tables (pyslice_amd/absorptive.py is the
// definition, absorptive_tables):
//     D     = exp(-2 pi^2 u^2 q^2)
//     V1    = Re ifft2(f)     / (dx^2 dy^2)
//     Vbar1 = Re ifft2(f D)   / (dx^2 dy^2)
//     Om1   = 1/2 (Re ifft2(D fft2(V1^2)) - Vbar1^2)
//     g     = Re fft2(Om1) dx^2 dy^2
// The kernels here are the pointwise steps between the transforms (fft2_inplace, batch = the species) and the epilogue that turns the
// two real stacks into t.  f and f D are real and even, so one complex transform carries both: W = f + i f D -> V1 + i Vbar1.
#pragma once
#include <hip/hip_runtime.h>
#include "potential.h"

namespace msl {

// ff = f D (float64, rounded once) and W = f + i f D on the (nx, ny) grid of every species; u_by_Z: rms width per atomic number.
// The Kirkland sum is formfactor_kernel's, term by term.
__global__ void absorptive_formfactor_kernel(float* __restrict__ ff, float2* __restrict__ W, const double* __restrict__ abcd,
                                             const double* __restrict__ u_by_Z, const int* __restrict__ species, int n_species, int nx,
                                             int ny, double inv_lx, double inv_ly) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long npix = (long long)nx * ny;
    if (i >= npix * n_species) return;
    const int sp = (int)(i / npix);
    const long long p = i - (long long)sp * npix;
    const int mx = (int)(p / ny), my = (int)(p - (long long)mx * ny);
    const double kx = signed_freq(mx, nx) * inv_lx, ky = signed_freq(my, ny) * inv_ly;
    const double q2 = kx * kx + ky * ky;
    const double* t = abcd + (size_t)(species[sp] - 1) * 12;
    double s1 = 0.0, s2 = 0.0;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        s1 += t[j * 4 + 0] / (q2 + t[j * 4 + 1]);
        s2 += t[j * 4 + 2] * exp(-t[j * 4 + 3] * q2);
    }
    const double f = s1 + s2, u = u_by_Z[species[sp] - 1];
    const double fd = f * exp(-2.0 * M_PI * M_PI * u * u * q2);
    ff[i] = (float)fd;
    if (W) W[i] = make_float2((float)f, (float)fd);
}

// W = V1 + i Vbar1  ->  vb2 = Vbar1^2,  W = V1^2
__global__ void absorptive_square_kernel(float2* __restrict__ W, float* __restrict__ vb2, long long n) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float2 w = W[i];
    vb2[i] = w.y * w.y;
    W[i] = make_float2(w.x * w.x, 0.f);
}

// W *= D(q^2) of its species (the factor in float64, rounded once)
__global__ void absorptive_damp_kernel(float2* __restrict__ W, const double* __restrict__ u_by_Z, const int* __restrict__ species,
                                       int n_species, int nx, int ny, double inv_lx, double inv_ly) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long npix = (long long)nx * ny;
    if (i >= npix * n_species) return;
    const int sp = (int)(i / npix);
    const long long p = i - (long long)sp * npix;
    const int mx = (int)(p / ny), my = (int)(p - (long long)mx * ny);
    const double kx = signed_freq(mx, nx) * inv_lx, ky = signed_freq(my, ny) * inv_ly;
    const double u = u_by_Z[species[sp] - 1];
    const float d = (float)exp(-2.0 * M_PI * M_PI * u * u * (kx * kx + ky * ky));
    const float2 w = W[i];
    W[i] = make_float2(w.x * d, w.y * d);
}

// W = <V1^2>  ->  W = Om1 = 1/2 (Re W - Vbar1^2)
__global__ void absorptive_variance_kernel(float2* __restrict__ W, const float* __restrict__ vb2, long long n) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    W[i] = make_float2(0.5f * (W[i].x - vb2[i]), 0.f);
}

// ffa = Re W * scale  (g = Re fft2(Om1) dx^2 dy^2)
__global__ void absorptive_real_kernel(float* __restrict__ ffa, const float2* __restrict__ W, long long n, float scale) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    ffa[i] = W[i].x * scale;
}

__device__ __forceinline__ float2 absorptive_t(float v, float om, float sigma_over_pi, float sigma2) {
    float sn, cs;
    sincospif(sigma_over_pi * v, &sn, &cs);
    const float a = expf(-sigma2 * om);
    return make_float2(a * cs, a * sn);
}

// t = exp(-sigma^2 Omega) (cos sigma Vbar, sin sigma Vbar) over n pixels, four per thread: 4 + 4 bytes in, 8 out per pixel, in 16-byte
// accesses when VEC (the host sets it when all three bases are 16-byte aligned); the last n % 4 pixels and the unaligned case go
// pixel by pixel.  ABSORB false: Omega is not read and |t| = 1.  sigma_over_pi and sigma2 are formed in double by the caller.
template <bool ABSORB, bool VEC>
__global__ void transmission_absorptive_kernel(float2* __restrict__ t, const float* __restrict__ V, const float* __restrict__ Om, long long n,
                                               float sigma_over_pi, float sigma2) {
    const long long i4 = ((long long)blockIdx.x * blockDim.x + threadIdx.x) * 4;
    if (i4 >= n) return;
    if (VEC && i4 + 4 <= n) {
        const float4 v = *reinterpret_cast<const float4*>(V + i4);
        float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
        if (ABSORB) o = *reinterpret_cast<const float4*>(Om + i4);
        const float2 a = absorptive_t(v.x, o.x, sigma_over_pi, sigma2), b = absorptive_t(v.y, o.y, sigma_over_pi, sigma2);
        const float2 c = absorptive_t(v.z, o.z, sigma_over_pi, sigma2), d = absorptive_t(v.w, o.w, sigma_over_pi, sigma2);
        *reinterpret_cast<float4*>(t + i4) = make_float4(a.x, a.y, b.x, b.y);
        *reinterpret_cast<float4*>(t + i4 + 2) = make_float4(c.x, c.y, d.x, d.y);
        return;
    }
    const long long end = i4 + 4 < n ? i4 + 4 : n;
    for (long long i = i4; i < end; ++i) t[i] = absorptive_t(V[i], ABSORB ? Om[i] : 0.f, sigma_over_pi, sigma2);
}

}  // namespace msl
