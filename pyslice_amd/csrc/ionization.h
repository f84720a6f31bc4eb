// Element maps: channelling-weighted ionisation signal per element (pyslice_amd/ionization.py is the
// definition).  For channel e (an atomic number, a Gaussian of rms width w_e and a cross-section c_e) and slice s
//     W_e,s(r) = Re ifft2( c_e exp(-2 pi^2 w_e^2 |k|^2) sum_{i in A_e,s} exp(-2 pi i k r_i) ) / (dx dy)
//     I[p, e, s] = sum_r |psi_p,s(r)|^2 W_e,s(r) / sum_r |psi_p,0(r)|^2,      psi_p,s the wave arriving at slice s.
// W is the structure-factor sum of the potential build with a table that is non-zero for one species only (ion_table_kernel), through
// the build's own launchers.  The kernels here: that table, the reduction of the slice loop and its finishing sum.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace msl {

constexpr int ION_MAX = 8;                  // channels
constexpr int ION_SL = 2;                   // pixel pairs per lane of a tile
constexpr int ION_TILE = 256 * ION_SL;      // pixel pairs per tile: 1024 pixels, the reach of a float32 partial

// tab (n_species, nx, ny) f32 on the fftfreq grid: amp exp(-2 pi^2 w^2 |k|^2) for species `sp`, zero for every other one (sp < 0: all
// zero).  amp = c dx dy: the build's inverse transform divides by dx^2 dy^2.
__global__ void ion_table_kernel(float* __restrict__ tab, int n_species, int sp, int nx, int ny, double inv_lx, double inv_ly, double w,
                                 double amp) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long npix = (long long)nx * ny;
    if (i >= npix * n_species) return;
    float v = 0.f;
    if ((int)(i / npix) == sp) {
        const long long p = i % npix;
        const int mx = (int)(p / ny), my = (int)(p - (long long)mx * ny);
        const double kx = (mx < (nx + 1) / 2 ? mx : mx - nx) * inv_lx, ky = (my < (ny + 1) / 2 ? my : my - ny) * inv_ly;
        v = (float)(amp * exp(-2.0 * M_PI * M_PI * w * w * (kx * kx + ky * ky)));
    }
    tab[i] = v;
}

// NE sums per lane -> the sums over the 64 lanes of the wave, in float32.  While more than one channel is left a lane gives half of
// its channels to its partner at distance o and takes the partner's share of the other half (NE / 2 + NE / 4 + .. shuffles instead
// of NE per distance); then the one channel it is left with goes over the remaining distances.  Afterwards a[0] of lane l holds
// channel ion_lane_channel<NE>(l).  The order of the additions is fixed: the same input gives the same bits.
template <int NE>
__device__ __forceinline__ void ion_wave_sum(float (&a)[NE], int lane) {
    int o = 1;
#pragma unroll
    for (int k = NE; k > 1; k >>= 1, o <<= 1) {
        const bool up = lane & o;
#pragma unroll
        for (int i = 0; i < k / 2; ++i) {
            const float send = up ? a[i] : a[i + k / 2], keep = up ? a[i + k / 2] : a[i];
            a[i] = keep + __shfl_xor(send, o, 64);
        }
    }
#pragma unroll
    for (; o < 64; o <<= 1) a[0] += __shfl_xor(a[0], o, 64);
}
template <int NE>
__device__ __forceinline__ int ion_lane_channel(int lane) {
    int c = 0, half = NE / 2;
#pragma unroll
    for (int o = 1; o < NE; o <<= 1, half >>= 1) c += (lane & o) ? half : 0;
    return c;
}

// The reduction.  psi: (P, nx, pitch) c64, natural order, the waves at their true scale; w: n <= NE images (nx, ny) f32, `w_es`
// values between two channels, already offset to the slice (the channels n .. NE - 1 of the template count as zero).  The pixels of an
// image are taken in pairs along y, ppr = (ny + 1) / 2 pairs per row (the second pixel of the last pair of an odd row does not
// exist), nx * ppr pairs per image in tiles of ION_TILE: a workgroup owns tile blockIdx.x and the images [blockIdx.y * pchunk,
// +pchunk).  It loads the weights of its pairs once, 2 NE values per slot into registers, and streams its images through them with
// the next image's loads in flight: every pixel of psi is read once and multiplied with all channels.  Per image |psi|^2 W is added
// in float32 over the at most 4 pixels of a lane, the 256 of a wave (ion_wave_sum) and the 1024 of the tile (through the LDS, two
// buffers, one barrier per image); thread e stores part[(tile * P + image) * NE + e] (float32).  ion_finish_kernel adds the tiles in
// float64.  VEC: pitch even and psi on 16 bytes -- one 16-byte load per pair; else two 8-byte loads.  No atomics.
template <int NE, bool VEC>
__global__ void __launch_bounds__(256) ion_reduce_kernel(const float2* __restrict__ psi, const float* __restrict__ w, long long w_es, int n,
                                                         int nx, int ny, int pitch, int P, int pchunk, float* __restrict__ part) {
    __shared__ float lds[2][4][NE];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int ppr = (ny + 1) >> 1;
    const long long pairs = (long long)nx * ppr;
    const long long tile = blockIdx.x;
    const long long image_stride = (long long)nx * pitch;

    long long off[ION_SL];              // element offset of the pair inside an image, -1: no such pair
    bool two[ION_SL];                   // the pair has its second pixel
    float c[ION_SL][2][NE];
#pragma unroll
    for (int s = 0; s < ION_SL; ++s) {
        const long long q = tile * ION_TILE + (long long)s * 256 + threadIdx.x;
        off[s] = -1; two[s] = false;
#pragma unroll
        for (int e = 0; e < NE; ++e) c[s][0][e] = c[s][1][e] = 0.f;
        if (q < pairs) {
            const int x = (int)(q / ppr), y = 2 * (int)(q - (long long)x * ppr);
            off[s] = (long long)x * pitch + y;
            two[s] = y + 1 < ny;
            const float* wp = w + (long long)x * ny + y;
#pragma unroll
            for (int e = 0; e < NE; ++e) {
                if (e < n) {
                    c[s][0][e] = wp[e * w_es];
                    if (two[s]) c[s][1][e] = wp[e * w_es + 1];
                }
            }
        }
    }

    auto load = [&](const float2* img, float4 (&v)[ION_SL]) {
#pragma unroll
        for (int s = 0; s < ION_SL; ++s) {
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
    const int my_channel = ion_lane_channel<NE>(lane);
    float4 vn[ION_SL];
    if (p0 < p1) load(psi + (long long)p0 * image_stride, vn);
    for (int p = p0; p < p1; ++p) {
        float4 v[ION_SL];
#pragma unroll
        for (int s = 0; s < ION_SL; ++s) v[s] = vn[s];
        if (p + 1 < p1) load(psi + (long long)(p + 1) * image_stride, vn);
        float acc[NE];
#pragma unroll
        for (int e = 0; e < NE; ++e) acc[e] = 0.f;
#pragma unroll
        for (int s = 0; s < ION_SL; ++s) {
            const float I0 = v[s].x * v[s].x + v[s].y * v[s].y, I1 = v[s].z * v[s].z + v[s].w * v[s].w;
#pragma unroll
            for (int e = 0; e < NE; ++e) acc[e] += I0 * c[s][0][e] + I1 * c[s][1][e];
        }
        ion_wave_sum<NE>(acc, lane);
        const int buf = (p - p0) & 1;
        if (lane < NE) lds[buf][wave][my_channel] = acc[0];
        __syncthreads();
        if ((int)threadIdx.x < NE) {
            const int e = threadIdx.x;
            part[(tile * P + p) * NE + e] = ((lds[buf][0][e] + lds[buf][1][e]) + lds[buf][2][e]) + lds[buf][3][e];
        }
    }
}

// acc[image * n + e] = sum over the tiles of part[tile][image][e] in float64, in tile order: one thread per (image, slot e < NE)
template <int NE>
__global__ void __launch_bounds__(256) ion_finish_kernel(const float* __restrict__ part, long long n_tiles, int P, int n,
                                                         double* __restrict__ acc) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long total = (long long)P * NE;
    if (i >= total) return;
    const int e = (int)(i % NE);
    if (e >= n) return;
    double s = 0.0;
    for (long long t = 0; t < n_tiles; ++t) s += (double)part[t * total + i];
    acc[(i / NE) * n + e] = s;
}

}  // namespace msl
