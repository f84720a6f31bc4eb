// TDS detector signal of the absorptive potential: what the absorption takes out of the elastic wave in
// slice s and a detector collects,
//     I[p, d, s] = sum_r |psi_p,s(r)|^2 w_d,s(r),     w_d,s = 1 - exp(-2 sigma^2 Omega_det,d,s),
// psi_p,s the wave arriving at slice s.  Omega_det is the structure-factor sum of the potential build with the detector-restricted
// tables (pyslice_amd/tds.py is the definition, tds_tables), M_d the detector's membership on the fftfreq grid:
//     V1M    = Re ifft2(M f)   / (dx^2 dy^2)        Vbar1M = Re ifft2(M f D) / (dx^2 dy^2)
//     Om1det = 1/2 (Re ifft2(D fft2(V1 V1M)) - Vbar1 Vbar1M)
//     g_det  = Re fft2(Om1det) dx^2 dy^2
// The kernels here: the two pointwise steps the tables add to absorptive.h's, the weight epilogue, and the reduction of the slice
// loop with its finishing sum.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace msl {

constexpr int TDS_MAX = 4;                  // detectors
constexpr int TDS_SL = 4;                   // pixel pairs per lane of a tile
constexpr int TDS_TILE = 256 * TDS_SL;      // pixel pairs per tile

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

// The reduction.  psi: (P, nx, pitch) c64, natural order, the waves at their true scale; w: (ND, nz, nx, ny) f32, `w_ds` values
// between two detectors, already offset to the slice.  The pixels of an image are taken in pairs along y, ppr = (ny + 1) / 2 pairs per
// row (the second pixel of the last pair of an odd row does not exist), nx * ppr pairs per image in tiles of TDS_TILE: a workgroup
// owns tile blockIdx.x, a run of whole and partial rows, and the images [blockIdx.y * pchunk, +pchunk).  It loads the weights of its
// pairs once, 2 ND values per slot into registers, and streams its images through them with the next image's loads in flight (as
// row_pass_pf_kernel streams its probes through t_z): |psi|^2 w in f32 per pixel, added in float64 per lane; per image the ND sums
// go across the wave by shuffles, across the four waves through the LDS (two buffers, one barrier per image), and thread d stores
// part[(tile * P + image) * ND + d].  VEC: pitch even and psi on 16 bytes -- one 16-byte load per pair; else two 8-byte loads.
// No atomics: the same input gives bitwise the same output, whatever pchunk.
template <int ND, bool VEC>
__global__ void __launch_bounds__(256) tds_reduce_kernel(const float2* __restrict__ psi, const float* __restrict__ w, long long w_ds,
                                                         int nx, int ny, int pitch, int P, int pchunk, double* __restrict__ part) {
    __shared__ double lds[2][4][ND];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int ppr = (ny + 1) >> 1;
    const long long pairs = (long long)nx * ppr;
    const long long tile = blockIdx.x;
    const long long image_stride = (long long)nx * pitch;

    long long off[TDS_SL];              // element offset of the pair inside an image, -1: no such pair
    bool two[TDS_SL];                   // the pair has its second pixel
    float c[TDS_SL][2][ND];
#pragma unroll
    for (int s = 0; s < TDS_SL; ++s) {
        const long long q = tile * TDS_TILE + (long long)s * 256 + threadIdx.x;
        off[s] = -1; two[s] = false;
#pragma unroll
        for (int d = 0; d < ND; ++d) c[s][0][d] = c[s][1][d] = 0.f;
        if (q < pairs) {
            const int x = (int)(q / ppr), y = 2 * (int)(q - (long long)x * ppr);
            off[s] = (long long)x * pitch + y;
            two[s] = y + 1 < ny;
            const float* wp = w + (long long)x * ny + y;
#pragma unroll
            for (int d = 0; d < ND; ++d) {
                c[s][0][d] = wp[d * w_ds];
                if (two[s]) c[s][1][d] = wp[d * w_ds + 1];
            }
        }
    }

    auto load = [&](const float2* img, float4 (&v)[TDS_SL]) {
#pragma unroll
        for (int s = 0; s < TDS_SL; ++s) {
            v[s] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (off[s] < 0) continue;
            if constexpr (VEC) {
                const float4 t = *reinterpret_cast<const float4*>(img + off[s]);     // (a pad pixel behind an odd row is read and dropped)
                v[s].x = t.x; v[s].y = t.y;
                if (two[s]) { v[s].z = t.z; v[s].w = t.w; }
            } else {
                const float2 a = img[off[s]];
                v[s].x = a.x; v[s].y = a.y;
                if (two[s]) { const float2 b = img[off[s] + 1]; v[s].z = b.x; v[s].w = b.y; }
            }
        }
    };

    const int p0 = blockIdx.y * pchunk, p1 = min(P, p0 + pchunk);
    float4 vn[TDS_SL];
    if (p0 < p1) load(psi + (long long)p0 * image_stride, vn);
    for (int p = p0; p < p1; ++p) {
        float4 v[TDS_SL];
#pragma unroll
        for (int s = 0; s < TDS_SL; ++s) v[s] = vn[s];
        if (p + 1 < p1) load(psi + (long long)(p + 1) * image_stride, vn);
        double acc[ND];
#pragma unroll
        for (int d = 0; d < ND; ++d) acc[d] = 0.0;
#pragma unroll
        for (int s = 0; s < TDS_SL; ++s) {
            const float I0 = v[s].x * v[s].x + v[s].y * v[s].y, I1 = v[s].z * v[s].z + v[s].w * v[s].w;
#pragma unroll
            for (int d = 0; d < ND; ++d) acc[d] += (double)(I0 * c[s][0][d]) + (double)(I1 * c[s][1][d]);
        }
#pragma unroll
        for (int d = 0; d < ND; ++d) {
#pragma unroll
            for (int o = 32; o >= 1; o >>= 1) acc[d] += __shfl_xor(acc[d], o, 64);
        }
        const int buf = (p - p0) & 1;
        if (lane == 0) {
#pragma unroll
            for (int d = 0; d < ND; ++d) lds[buf][wave][d] = acc[d];
        }
        __syncthreads();
        if ((int)threadIdx.x < ND) {
            const int d = threadIdx.x;
            part[(tile * P + p) * ND + d] = ((lds[buf][0][d] + lds[buf][1][d]) + lds[buf][2][d]) + lds[buf][3][d];
        }
    }
}

// acc[image * n + d] = sum over the tiles of part[tile][image][d], in tile order: one thread per (image, slot d < ND)
template <int ND>
__global__ void __launch_bounds__(256) tds_finish_kernel(const double* __restrict__ part, long long n_tiles, int P, int n,
                                                         double* __restrict__ acc) {
    const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long total = (long long)P * ND;
    if (e >= total) return;
    const int d = (int)(e % ND);
    if (d >= n) return;
    double s = 0.0;
    for (long long t = 0; t < n_tiles; ++t) s += part[t * total + e];
    acc[(e / ND) * n + d] = s;
}

}  // namespace msl
