// TDS detector signal of the absorptive potential: what the absorption takes out of the elastic wave in
// slice s and a detector collects,
//     I[p, d, s] = sum_r |psi_p,s(r)|^2 w_d,s(r),     w_d,s = 1 - exp(-2 sigma^2 Omega_det,d,s),
// psi_p,s the wave arriving at slice s.  Omega_det is the structure-factor sum of the potential build with the detector-restricted
// tables (pyslice_amd/tds.py is the definition, tds_tables), M_d the detector's membership on the fftfreq grid:
//     V1M    = Re ifft2(M f)   / (dx^2 dy^2)        Vbar1M = Re ifft2(M f D) / (dx^2 dy^2)
//     Om1det = 1/2 (Re ifft2(D fft2(V1 V1M)) - Vbar1 Vbar1M)
//     g_det  = Re fft2(Om1det) dx^2 dy^2
// The kernels here: the two pointwise steps the tables add to absorptive.h's and the weight epilogue.  The reduction of the slice loop
// and its finishing sum are slice_sums.h's, with the policy TdsSums (float64 sums, 1024 pixel pairs per tile).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace msl {

constexpr int TDS_MAX = 4;                  // detectors

// WM = M_d F of every species: F = f + i f D (n_species, nx, ny), bits (nx, ny) in fft order, bit d = detector d
__global__ void tds_mask_kernel(float2* __restrict__ WM, const float2* __restrict__ F, const uint16_t* __restrict__ bits, int d,
                                long long npix, long long n) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    WM[i] = ((bits[i % npix] >> d) & 1u) ? F[i] : make_float2(0.f, 0.f);
}

// W0 = V1 + i Vbar1, WM = V1M + i Vbar1M  ->  vb = Vbar1 Vbar1M,  WM = V1 V1M   (absorptive_square_kernel's step with the two
// detector terms; absorptive_variance_kernel then takes vb as it takes Vbar1^2)
__global__ void tds_product_kernel(float2* __restrict__ WM, const float2* __restrict__ W0, float* __restrict__ vb, long long n) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float2 a = W0[i], b = WM[i];
    vb[i] = a.y * b.y;
    WM[i] = make_float2(a.x * b.x, 0.f);
}

// The weight stack in place over n values, four per thread (16-byte accesses; the base is hipMalloc's, and the last n % 4 values go
// one by one).  From Omega_det: w = -expm1(-a Omega), a = 2 sigma^2 (ratio == 0).  From the weights of another beam (msl_set_beam):
// Omega a_old = -log1p(-w), so w' = -expm1(ratio log1p(-w)), ratio = a_new / a_old (a == 0 then).
__device__ __forceinline__ float tds_w(float v, float a, float ratio) {
    return ratio == 0.f ? -expm1f(-a * v) : -expm1f(ratio * log1pf(-v));
}
__global__ void tds_weight_kernel(float* __restrict__ w, long long n, float a, float ratio) {
    const long long i4 = ((long long)blockIdx.x * blockDim.x + threadIdx.x) * 4;
    if (i4 >= n) return;
    if (i4 + 4 <= n) {
        float4 v = *reinterpret_cast<const float4*>(w + i4);
        v.x = tds_w(v.x, a, ratio); v.y = tds_w(v.y, a, ratio); v.z = tds_w(v.z, a, ratio); v.w = tds_w(v.w, a, ratio);
        *reinterpret_cast<float4*>(w + i4) = v;
        return;
    }
    for (long long i = i4; i < n; ++i) w[i] = tds_w(w[i], a, ratio);
}

}  // namespace msl
