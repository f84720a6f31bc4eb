// Detector pass (msl_detect): STEM detector signals of every (row, detector) in one launch plus one float64 finishing launch.
//   out[row, d] = sum_k w_d(k) f_d(Psi[row, k]),   w_d(k) = bit d of mask[k],
//   f_d = |Psi|^2 (intensity), |Psi| (amplitude, haadf_data.py:50, 63), kx(k) |Psi|^2 (com_x) or ky(k) |Psi|^2 (com_y),
//   kx(k) = kx_tab[k / wy], ky(k) = ky_tab[k % wy] (the run's stored k axes).
// Rows of K stored pixels start every `ld` pixels; row r = b * count + j is frame slot t0 + j of probe b of a (B, T, ld) array.
//
// Pixel-tile-major: a workgroup owns one tile of TP = 64 * PX contiguous pixels and a block of rows.  Each wave turns the masks
// and axis values of its tile into per-pixel, per-detector coefficients c[p][d] = w_d(k) * (1 | kx | ky) ONCE, in registers, and
// then streams its rows through them: per pixel and detector one FMA on |Psi|^2 or |Psi|.  The detector description is read
// once per (tile, row block) instead of once per image, and every complex value is read from HBM once (16-byte loads when the
// rows start on 16 bytes).  PX = 64 / ND keeps the coefficient block at 64 VGPRs for ND = 4, 8 and 16 detector slots.
// Per (row, tile) the wave reduces its ND fp32 sums (over at most 1024 pixels) with a halving exchange, ND + log2(64/ND)
// shuffles instead of 6 ND, and stores them to a partial slab; detect_finish_kernel sums the slab in float64 in a fixed order.
// No atomics: the same input gives bitwise the same output.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace msl {

constexpr int DET_MAX = 16;

// MODE 0: every detector reads |Psi|^2 (intensity / com);  1: every detector reads |Psi| (amplitude);  2: mixed (amp_bits)
template <int ND, int MODE, bool VEC>
__global__ void __launch_bounds__(256) detect_tile_kernel(const float2* __restrict__ src, long long T, long long t0, long long count,
                                                          long long ld, long long K, long long rows, int rows_per_wg,
                                                          const uint16_t* __restrict__ mask, const float* __restrict__ kx_tab,
                                                          const float* __restrict__ ky_tab, int wy, uint32_t amp_bits,
                                                          uint32_t cx_bits, uint32_t cy_bits, float* __restrict__ part) {
    constexpr int PX = 64 / ND;                 // pixels per lane of a tile
    constexpr int TP = 64 * PX;                 // pixels per tile
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long tile = blockIdx.x, n_tiles = gridDim.x;
    const long long tile0 = tile * TP;
    const bool full = tile0 + TP <= K;
    // pixel of slot p of this lane: pairs of pixels per 16-byte load (VEC), else one pixel per 8-byte load; both coalesced
    auto pix = [&](int p) -> long long {
        return VEC ? tile0 + 2 * ((p >> 1) * 64 + lane) + (p & 1) : tile0 + (long long)p * 64 + lane;
    };

    float c[PX][ND];
#pragma unroll
    for (int p = 0; p < PX; ++p) {
        const long long k = pix(p);
        uint32_t m = 0;
        float kxv = 0.f, kyv = 0.f;
        if (k < K) {
            m = mask[k];
            const long long ix = k / wy;
            kxv = kx_tab[ix];
            kyv = ky_tab[k - ix * wy];
        }
#pragma unroll
        for (int d = 0; d < ND; ++d) {
            const float g = ((cx_bits >> d) & 1u) ? kxv : (((cy_bits >> d) & 1u) ? kyv : 1.f);
            c[p][d] = ((m >> d) & 1u) ? g : 0.f;
        }
    }

    const long long r0 = (long long)blockIdx.y * rows_per_wg;
    const long long r1 = min(rows, r0 + rows_per_wg);
    for (long long r = r0 + wave; r < r1; r += 4) {
        const long long b = r / count, j = r - b * count;
        const float2* row = src + (b * T + t0 + j) * ld;
        float2 z[PX];
        if constexpr (VEC) {
            const float4* row4 = reinterpret_cast<const float4*>(row);
#pragma unroll
            for (int q = 0; q < PX / 2; ++q) {
                const long long k = pix(2 * q);
                float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
                if (full || k + 1 < K) v = row4[k >> 1];
                else if (k < K) { const float2 s = row[k]; v.x = s.x; v.y = s.y; }
                z[2 * q] = make_float2(v.x, v.y);
                z[2 * q + 1] = make_float2(v.z, v.w);
            }
        } else {
#pragma unroll
            for (int p = 0; p < PX; ++p) {
                const long long k = pix(p);
                z[p] = (full || k < K) ? row[k] : make_float2(0.f, 0.f);
            }
        }
        float acc[ND];
#pragma unroll
        for (int d = 0; d < ND; ++d) acc[d] = 0.f;
#pragma unroll
        for (int p = 0; p < PX; ++p) {
            const float I = z[p].x * z[p].x + z[p].y * z[p].y;
            const float A = MODE == 0 ? 0.f : sqrtf(I);
#pragma unroll
            for (int d = 0; d < ND; ++d) {
                const float base = MODE == 0 ? I : (MODE == 1 ? A : (((amp_bits >> d) & 1u) ? A : I));
                acc[d] = fmaf(base, c[p][d], acc[d]);
            }
        }
        // halving exchange: after log2(ND) steps lane l holds detector l / (64 / ND) summed over the lanes that agree with it in
        // the upper bits; the remaining steps finish the sum over the other 64 / ND lanes
#pragma unroll
        for (int h = ND / 2, o = 32; h >= 1; h >>= 1, o >>= 1) {
            const bool up = (lane & o) != 0;
#pragma unroll
            for (int i = 0; i < h; ++i) {
                const float send = up ? acc[i] : acc[i + h];
                const float keep = up ? acc[i + h] : acc[i];
                acc[i] = keep + __shfl_xor(send, o, 64);
            }
        }
        float v = acc[0];
#pragma unroll
        for (int o = 32 / ND; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
        if ((lane & (64 / ND - 1)) == 0) part[(r * n_tiles + tile) * ND + lane / (64 / ND)] = v;
    }
}

// out[row * n + d] = sum over the tiles of part[row][tile][d], float64, one workgroup per row, fixed order
template <int ND>
__global__ void __launch_bounds__(256) detect_finish_kernel(const float* __restrict__ part, long long n_tiles, int n,
                                                            double* __restrict__ out) {
    __shared__ double lds[256];
    const long long row = blockIdx.x;
    const float* p = part + row * n_tiles * ND;
    const long long total = n_tiles * ND;
    double acc = 0.0;
    for (long long e = threadIdx.x; e < total; e += 256) acc += (double)p[e];      // element e belongs to detector e % ND == t % ND
    lds[threadIdx.x] = acc;
    __syncthreads();
    if ((int)threadIdx.x < n) {
        double s = 0.0;
        for (int i = threadIdx.x; i < 256; i += ND) s += lds[i];
        out[row * n + threadIdx.x] = s;
    }
}

}  // namespace msl
