// Imaging pass (msl_image_add): stored exit spectra -> objective lens -> inverse transform -> frame-accumulated image intensity.
//   I[first + b * stride](r) += weight * sum_{j < count} | ifft2( ifftshift(Psi[b, t0 + j]) * H )(r) |^2
//   H(k) = A(k) exp(-i chi(k)),   A = 1 for |k| < k_ap (strict, the probe kernel's rule) or without an aperture, else 0
// over a (B, T, ld) complex64 array of full-grid spectra fftshift(fft2(exit)), unnormalised, whose images start every `ld` pixels.
// Three launches per chunk of frames: lens_apply_kernel into the work buffer (psi's layout, image = j * B + b), the inverse
// transform of fft2_inplace in place, image_accumulate_kernel into the handle's (n_images, nx * ny) float64 accumulator.
//
// lens_apply_kernel: a lane owns one pixel (VEC: one column pair) of the UNSHIFTED (nx, ny) grid.  It evaluates H once -- kx, ky, the
// aperture test as probe_kspace_aberr_kernel (potential.h), the Cartesian float64 polynomial of chi in turns of aberration.h, reduced to
// one turn in float64 before the one float sincospif -- and reuses it for every image of the launch it walks.  Outside the aperture
// it stores zeros and neither reads the source nor does float64 work.  The source pixel of (mx, my) is ((mx + nx/2) % nx,
// (my + ny/2) % ny) of the shifted spectrum, which is ifftshift for odd lengths too.  VEC (16-byte loads and stores) needs ny and
// ny / 2 even (then the shifted column of an even column is even and the pair does not wrap), ld and the work pitch even and a
// 16-byte-aligned source; every other case takes one pixel per lane with 8-byte accesses.  Pad pixels (k >= nx * ny) are never read.
// image_accumulate_kernel: a lane owns one pixel (VEC: a pixel pair; ny and the work pitch even) of accumulator image
// first + b * stride and walks the frames of the chunk in order: fp32 |psi|^2, widened to float64, times the float64 weight, added.
// No atomics; the accumulator is read and written once per launch.  One call over [0, T) and calls over [0, s), [s, T) perform the
// same additions, and repeated sequences are bitwise equal.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "aberration.h"
#include "potential.h"

namespace msl {

// H at the unshifted pixel (mx, my); false outside the aperture (radius <= 0: no aperture)
__device__ __forceinline__ bool lens_transfer(int mx, int my, int nx, int ny, double kfreq_x, double kfreq_y, double radius, double wavelength,
                                              int has_chi, const ProbeAberrations& ab, float2* H) {
    const int fx = signed_freq(mx, nx), fy = signed_freq(my, ny);
    const double kx = fx * kfreq_x, ky = fy * kfreq_y;       // fftfreq value = index * (1/(n*d))
    if (radius > 0.0 && !(sqrt(kx * kx + ky * ky) < radius)) return false;
    if (!has_chi) { *H = make_float2(1.f, 0.f); return true; }
    double t = -aberration_chi_turns(wavelength * kx, wavelength * ky, ab, ab.a[0]);
    t -= rint(t);
    float sn, cs;
    sincospif((float)(2.0 * t), &sn, &cs);
    *H = make_float2(cs, sn);
    return true;
}

__device__ __forceinline__ float2 lens_mul(float2 v, float2 H) { return make_float2(v.x * H.x - v.y * H.y, v.x * H.y + v.y * H.x); }

// src: frame t0 of probe 0; image = j * B + b reads frame j of probe b.  grid.x covers the pixels (VEC: column pairs), grid.y strides
// over the images.
template <bool VEC>
__global__ void __launch_bounds__(256) lens_apply_kernel(const float2* __restrict__ src, long long B, long long T, long long ld, long long images,
                                                         int nx, int ny, int pitch, double kfreq_x, double kfreq_y, double radius,
                                                         double wavelength, int has_chi, ProbeAberrations ab, float2* __restrict__ work) {
    constexpr int PXL = VEC ? 2 : 1;
    const int cols = ny / PXL;                  // VEC: ny is a multiple of 4
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long long)nx * cols) return;
    const int mx = (int)(i / cols), my = (int)(i - (long long)mx * cols) * PXL;
    float2 H0 = make_float2(0.f, 0.f), H1 = make_float2(0.f, 0.f);
    const bool in0 = lens_transfer(mx, my, nx, ny, kfreq_x, kfreq_y, radius, wavelength, has_chi, ab, &H0);
    bool in1 = false;
    if constexpr (VEC) in1 = lens_transfer(mx, my + 1, nx, ny, kfreq_x, kfreq_y, radius, wavelength, has_chi, ab, &H1);
    int sx = mx + nx / 2, sy = my + ny / 2;
    if (sx >= nx) sx -= nx;
    if (sy >= ny) sy -= ny;
    const long long soff = (long long)sx * ny + sy, image_stride = (long long)nx * pitch;
    float2* dst = work + (long long)mx * pitch + my;
    if (!in0 && !in1) {
        for (long long img = blockIdx.y; img < images; img += gridDim.y) {
            if constexpr (VEC) *reinterpret_cast<float4*>(dst + img * image_stride) = make_float4(0.f, 0.f, 0.f, 0.f);
            else dst[img * image_stride] = make_float2(0.f, 0.f);
        }
        return;
    }
#pragma unroll 4
    for (long long img = blockIdx.y; img < images; img += gridDim.y) {
        const long long j = img / B, b = img - j * B;
        const float2* s = src + (b * T + j) * ld + soff;
        if constexpr (VEC) {
            const float4 v = *reinterpret_cast<const float4*>(s);
            const float2 o0 = lens_mul(make_float2(v.x, v.y), H0), o1 = lens_mul(make_float2(v.z, v.w), H1);      // (H = 0 outside)
            *reinterpret_cast<float4*>(dst + img * image_stride) = make_float4(in0 ? o0.x : 0.f, in0 ? o0.y : 0.f, in1 ? o1.x : 0.f, in1 ? o1.y : 0.f);
        } else {
            dst[img * image_stride] = lens_mul(*s, H0);
        }
    }
}

// work: (count * B, nx, pitch) of the chunk, image = j * B + b; acc: image 0 of the accumulator, nx * ny float64 per image
template <bool VEC>
__global__ void __launch_bounds__(256) image_accumulate_kernel(const float2* __restrict__ work, long long B, int count, int nx, int ny, int pitch,
                                                               double weight, long long first, long long stride, double* __restrict__ acc) {
    constexpr int PXL = VEC ? 2 : 1;
    const int cols = ny / PXL;                  // VEC: ny is even
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long long)nx * cols) return;
    const int mx = (int)(i / cols), my = (int)(i - (long long)mx * cols) * PXL;
    const long long npix = (long long)nx * ny, image_stride = (long long)nx * pitch;
    const float2* w0 = work + (long long)mx * pitch + my;
    for (long long b = blockIdx.y; b < B; b += gridDim.y) {
        double* a = acc + (first + b * stride) * npix + (long long)mx * ny + my;
        const float2* w = w0 + b * image_stride;
        if constexpr (VEC) {
            double2 s = *reinterpret_cast<double2*>(a);
#pragma unroll 4
            for (int j = 0; j < count; ++j) {
                const float4 v = *reinterpret_cast<const float4*>(w + (long long)j * B * image_stride);
                const float f0 = v.x * v.x + v.y * v.y, f1 = v.z * v.z + v.w * v.w;
                s.x += (double)f0 * weight;
                s.y += (double)f1 * weight;
            }
            *reinterpret_cast<double2*>(a) = s;
        } else {
            double s = a[0];
#pragma unroll 4
            for (int j = 0; j < count; ++j) {
                const float2 v = w[(long long)j * B * image_stride];
                const float f0 = v.x * v.x + v.y * v.y;
                s += (double)f0 * weight;
            }
            a[0] = s;
        }
    }
}

}  // namespace msl
