// Spectrum-detector pass (msl_spectrum_detect): the detector signals of every (probe, frequency) row of a TACAW intensity in one
// launch plus the float64 finishing launch of detect.h.
//   out[row, d] = sum_k w_d(k) I[row, k],   w_d(k) = bit d of mask[k]  (the memberships of msl_set_detectors, intensity signals only).
// Rows of K stored float32 pixels start every `ld` pixels; row r = b * count + j is frequency bin f0 + j of probe b of a (B, F, ld) array.
//
// The design is detect_tile_kernel's (detect.h), on real input: a workgroup owns one tile of TP = 64 * PX contiguous pixels and a
// block of rows.  Each wave turns the membership bits of its tile into per-pixel, per-detector 0/1 coefficients ONCE, in registers
// (PX = 64 / ND keeps them at 64 VGPRs for ND = 4, 8 and 16 detector slots), and then streams its rows through them: per pixel and
// detector one FMA.  D detectors cost one pass over the intensity instead of the D passes (and D host round trips) of
// msl_tacaw_spectrum with one byte mask each.  Every float is read from HBM once, VW pixels per load: 16 bytes when the rows start
// on 16 bytes, else 8 or 4; a group of VW pixels that crosses K falls back to scalar loads of the pixels below K, so the pad pixels
// [K, ld) are never read.  Per (row, tile) the wave reduces its ND fp32 sums (over at most 1024 pixels, all addends non-negative)
// with the halving exchange of detect.h and stores them to the partial slab part[row][tile][ND], the layout detect_finish_kernel
// sums in float64 in a fixed order.  No atomics: the same input gives bitwise the same output.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace msl {

template <int ND, int VW>
__global__ void __launch_bounds__(256) spectrum_tile_kernel(const float* __restrict__ src, long long F, long long f0, long long count,
                                                            long long ld, long long K, long long rows, int rows_per_wg,
                                                            const uint16_t* __restrict__ mask, float* __restrict__ part) {
    constexpr int PX = 64 / ND;                 // pixels per lane of a tile
    constexpr int TP = 64 * PX;                 // pixels per tile
    static_assert(PX % VW == 0, "whole loads per lane");
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long tile = blockIdx.x, n_tiles = gridDim.x;
    const long long tile0 = tile * TP;
    const bool full = tile0 + TP <= K;
    // pixel of slot p of this lane: VW neighbouring pixels per load, the loads of a wave coalesced
    auto pix = [&](int p) -> long long { return tile0 + (long long)VW * ((p / VW) * 64 + lane) + (p % VW); };

    float c[PX][ND];
#pragma unroll
    for (int p = 0; p < PX; ++p) {
        const long long k = pix(p);
        const uint32_t m = k < K ? mask[k] : 0u;
#pragma unroll
        for (int d = 0; d < ND; ++d) c[p][d] = ((m >> d) & 1u) ? 1.f : 0.f;
    }

    const long long r0 = (long long)blockIdx.y * rows_per_wg;
    const long long r1 = min(rows, r0 + rows_per_wg);
    for (long long r = r0 + wave; r < r1; r += 4) {
        const long long b = r / count, j = r - b * count;
        const float* row = src + (b * F + f0 + j) * ld;
        float v[PX];
#pragma unroll
        for (int q = 0; q < PX / VW; ++q) {
            const long long k = pix(q * VW);
            float t[VW];
            if (full || k + VW - 1 < K) {
                if constexpr (VW == 4) {
                    const float4 w = *reinterpret_cast<const float4*>(row + k);
                    t[0] = w.x; t[1] = w.y; t[2] = w.z; t[3] = w.w;
                } else if constexpr (VW == 2) {
                    const float2 w = *reinterpret_cast<const float2*>(row + k);
                    t[0] = w.x; t[1] = w.y;
                } else {
                    t[0] = row[k];
                }
            } else {
#pragma unroll
                for (int e = 0; e < VW; ++e) t[e] = k + e < K ? row[k + e] : 0.f;
            }
#pragma unroll
            for (int e = 0; e < VW; ++e) v[q * VW + e] = t[e];
        }
        float acc[ND];
#pragma unroll
        for (int d = 0; d < ND; ++d) acc[d] = 0.f;
#pragma unroll
        for (int p = 0; p < PX; ++p) {
#pragma unroll
            for (int d = 0; d < ND; ++d) acc[d] = fmaf(v[p], c[p][d], acc[d]);
        }
        // halving exchange (detect.h): after log2(ND) steps lane l holds detector l / (64 / ND) summed over the lanes that agree
        // with it in the upper bits; the remaining steps finish the sum over the other 64 / ND lanes
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
        float s = acc[0];
#pragma unroll
        for (int o = 32 / ND; o >= 1; o >>= 1) s += __shfl_xor(s, o, 64);
        if ((lane & (64 / ND - 1)) == 0) part[(r * n_tiles + tile) * ND + lane / (64 / ND)] = s;
    }
}

}  // namespace msl
