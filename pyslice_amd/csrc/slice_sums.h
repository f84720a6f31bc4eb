// Per-slice sums of the slice loop (DESIGN.md sections 4.23 and 4.27): for the wave psi_p,s arriving at slice s and a handful of real
// weight images w_c,s
//     I[p, c, s] = sum_r |psi_p,s(r)|^2 w_c,s(r).
// The TDS detector signal (tds.h: c a detector) and the element maps (ionization.h: c a channel) are this sum.  One tile kernel and one
// finishing sum serve both; a signal is a policy struct S that says what its measurements settled (profiles/tds_detector.txt,
// profiles/element_signals.txt):
//     acc_t      the type of the sums of a lane, a wave and a tile, and of the slab of partials
//     SL, TILE   pixel pairs per lane and per tile of 256 lanes
//     add        one pixel pair into a lane's sum: the products |psi|^2 w in f32, the sum in acc_t
//     GUARD_N    the weights of the template slots n .. N - 1 are not read and count as zero (else n is not looked at: N == n)
//     to_lds     the N sums of the 64 lanes of a wave -> slot(0 .. N - 1), the wave's places in the LDS
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace msl {

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

// TDS: float64 from the lane on, 4 pairs per lane (1024 per tile), N = the detector count; a full butterfly per detector, lane 0 writes
struct TdsSums {
    using kernel_policy = TdsSums;      // (what a host-side descriptor derived from this instantiates the kernels with)
    using acc_t = double;
    static constexpr int SL = 4, TILE = 256 * SL;
    static constexpr bool GUARD_N = false;
    static __device__ __forceinline__ void add(double& a, float I0, float c0, float I1, float c1) { a += (double)(I0 * c0) + (double)(I1 * c1); }
    template <int N, typename Slot>
    static __device__ __forceinline__ void to_lds(double (&a)[N], int lane, Slot&& slot) {
#pragma unroll
        for (int d = 0; d < N; ++d) {
#pragma unroll
            for (int o = 32; o >= 1; o >>= 1) a[d] += __shfl_xor(a[d], o, 64);
        }
        if (lane == 0) {
#pragma unroll
            for (int d = 0; d < N; ++d) slot(d) = a[d];
        }
    }
};

// Ionisation: float32 up to the tile, 2 pairs per lane (512 per tile: 1024 pixels, the reach of a float32 partial), N = the next power
// of two above the channel count; ion_wave_sum, and the lanes < N write the channel they are left with
struct IonSums {
    using kernel_policy = IonSums;
    using acc_t = float;
    static constexpr int SL = 2, TILE = 256 * SL;
    static constexpr bool GUARD_N = true;
    static __device__ __forceinline__ void add(float& a, float I0, float c0, float I1, float c1) { a += I0 * c0 + I1 * c1; }
    template <int N, typename Slot>
    static __device__ __forceinline__ void to_lds(float (&a)[N], int lane, Slot&& slot) {
        const int channel = ion_lane_channel<N>(lane);
        ion_wave_sum<N>(a, lane);
        if (lane < N) slot(channel) = a[0];
    }
};

// The reduction.  psi: (P, nx, pitch) c64, natural order, the waves at their true scale; w: n images (nx, ny) f32, `w_cs` values
// between two of them, already offset to the slice.  The pixels of an image are taken in pairs along y, ppr = (ny + 1) / 2 pairs per
// row (the second pixel of the last pair of an odd row does not exist), nx * ppr pairs per image in tiles of S::TILE: a workgroup
// owns tile blockIdx.x, a run of whole and partial rows, and the images [blockIdx.y * pchunk, +pchunk).  It loads the weights of its
// pairs once, 2 N values per slot into registers, and streams its images through them with the next image's loads in flight (as
// row_pass_pf_kernel streams its probes through t_z): every pixel of psi is read once and multiplied with all weights, |psi|^2 w in
// f32 per pixel, added in acc_t per lane; per image the N sums go across the wave by shuffles (S::to_lds), across the four waves
// through the LDS (two buffers, one barrier per image), and thread c stores part[(tile * P + image) * N + c].  VEC: pitch even and psi
// on 16 bytes -- one 16-byte load per pair; else two 8-byte loads.  No atomics: the same input gives bitwise the same output,
// whatever pchunk.
template <class S, int N, bool VEC>
__global__ void __launch_bounds__(256) slice_sums_kernel(const float2* __restrict__ psi, const float* __restrict__ w, long long w_cs, int n,
                                                         int nx, int ny, int pitch, int P, int pchunk, typename S::acc_t* __restrict__ part) {
    using acc_t = typename S::acc_t;
    constexpr int SL = S::SL;
    __shared__ acc_t lds[2][4][N];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int ppr = (ny + 1) >> 1;
    const long long pairs = (long long)nx * ppr;
    const long long tile = blockIdx.x;
    const long long image_stride = (long long)nx * pitch;

    long long off[SL];                  // element offset of the pair inside an image, -1: no such pair
    bool two[SL];                       // the pair has its second pixel
    float c[SL][2][N];
#pragma unroll
    for (int s = 0; s < SL; ++s) {
        const long long q = tile * S::TILE + (long long)s * 256 + threadIdx.x;
        off[s] = -1; two[s] = false;
#pragma unroll
        for (int k = 0; k < N; ++k) c[s][0][k] = c[s][1][k] = 0.f;
        if (q < pairs) {
            const int x = (int)(q / ppr), y = 2 * (int)(q - (long long)x * ppr);
            off[s] = (long long)x * pitch + y;
            two[s] = y + 1 < ny;
            const float* wp = w + (long long)x * ny + y;
#pragma unroll
            for (int k = 0; k < N; ++k) {
                if (!S::GUARD_N || k < n) {
                    c[s][0][k] = wp[k * w_cs];
                    if (two[s]) c[s][1][k] = wp[k * w_cs + 1];
                }
            }
        }
    }

    auto load = [&](const float2* img, float4 (&v)[SL]) {
#pragma unroll
        for (int s = 0; s < SL; ++s) {
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
    float4 vn[SL];
    if (p0 < p1) load(psi + (long long)p0 * image_stride, vn);
    for (int p = p0; p < p1; ++p) {
        float4 v[SL];
#pragma unroll
        for (int s = 0; s < SL; ++s) v[s] = vn[s];
        if (p + 1 < p1) load(psi + (long long)(p + 1) * image_stride, vn);
        acc_t acc[N];
#pragma unroll
        for (int k = 0; k < N; ++k) acc[k] = 0;
#pragma unroll
        for (int s = 0; s < SL; ++s) {
            const float I0 = v[s].x * v[s].x + v[s].y * v[s].y, I1 = v[s].z * v[s].z + v[s].w * v[s].w;
#pragma unroll
            for (int k = 0; k < N; ++k) S::add(acc[k], I0, c[s][0][k], I1, c[s][1][k]);
        }
        const int buf = (p - p0) & 1;
        S::template to_lds<N>(acc, lane, [&](int k) -> acc_t& { return lds[buf][wave][k]; });
        __syncthreads();
        if ((int)threadIdx.x < N) {
            const int k = threadIdx.x;
            part[(tile * P + p) * N + k] = ((lds[buf][0][k] + lds[buf][1][k]) + lds[buf][2][k]) + lds[buf][3][k];
        }
    }
}

// acc[image * n + c] = sum over the tiles of part[tile][image][c] in float64, in tile order: one thread per (image, slot c < N)
template <typename T, int N>
__global__ void __launch_bounds__(256) slice_sums_finish_kernel(const T* __restrict__ part, long long n_tiles, int P, int n,
                                                                double* __restrict__ acc) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long total = (long long)P * N;
    if (i >= total) return;
    const int c = (int)(i % N);
    if (c >= n) return;
    double s = 0.0;
    for (long long t = 0; t < n_tiles; ++t) s += (double)part[t * total + i];
    acc[(i / N) * n + c] = s;
}

}  // namespace msl
