// Ensembles of member probes per scan position (partial coherence of the probe; the definition is pyslice_amd/coherence.py).
// Position q of a scan is G waves of the batch, b = q * G + g, member g built at its own offset and defocus and weighted w_g.
//
// msl_set_probe_members builds the probes with probe_kspace_aberr_kernel<true> (potential.h): the C10 coefficient of the polynomial is
//   taken per probe from a device array, a0[p] = (C10 + defocus[p]) / (2 lambda); everything else is that one kernel body.
//
// diffract_members_kernel (msl_diffract_members, msl_dose_add_members): diffract_kernel's pattern pass with the G members of a
//   position folded on the device,
//     out[(q * mx + ix) * my + iy] = sum_{g < G} w_g * D[q * G + g, ix, iy],      D = msl_diffract's result for that wave.
//   Strip-major like diffract_kernel, a strip being one row of bins of one POSITION: the workgroup walks the G members of the strip
//   in order and forms, per member, the column sums with diffract_kernel's own walk (strip_columns, diffract.h) and the bin sums with
//   its helpers, in the same three modes with the same owner lane; the owner then adds w_g * that sum to the bin's float64 total -- one
//   rounded multiply and one rounded add, never contracted, so the result is bit for bit the host's float64 sum of w_g * D_g in member
//   order.  Every complex value is read once, 1 / G of msl_diffract's output is written, no atomics.  ACC adds the totals to out
//   (msl_dose_add_members).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "diffract.h"

namespace msl {

constexpr int MEMBERS_MAX = 128;                // include/mslice.h: MSL_MEMBERS_MAX

// the member weights, passed to the kernel by value (1 KB of kernel arguments: no upload, nothing of the caller's read after the launch)
struct MemberWeights {
    double w[MEMBERS_MAX];
};

// total + w * v, the product and the sum each rounded on their own
__device__ __forceinline__ double member_add(double total, double w, double v) {
#pragma clang fp contract(off)
    const double wv = w * v;
    return total + wv;
}

template <int MODE, bool VEC, bool ACC>
__global__ void __launch_bounds__(256) diffract_members_kernel(const float2* __restrict__ src, long long T, long long t0, int count, long long ld,
                                                               int wx, int wy, int bx, int by, int G, MemberWeights weights,
                                                               long long strips, int strips_per_wg, double* __restrict__ out) {
    extern __shared__ double mem_lds[];         // DIFF_LDS: the wy column sums of one member's strip, then the my totals of the strip
    constexpr int PXL = VEC ? 2 : 1;            // columns per lane and chunk
    const int mx = wx / bx, my = wy / by;
    const int nt = blockDim.x, tid = threadIdx.x;
    const int rows = count * bx;
    const long long frame_step = ld - (long long)bx * wy;       // from behind the last row of a frame's strip to the next frame's first
    const long long member_step = T * ld;                        // from a member's wave to the next member's
    const long long s0 = (long long)blockIdx.x * strips_per_wg;
    const long long s1 = min(strips, s0 + strips_per_wg);
    double* const mem_col = mem_lds;
    double* const mem_tot = mem_lds + wy;
    for (long long s = s0; s < s1; ++s) {
        const long long q = s / mx;
        const int ix = (int)(s - q * mx);
        const float2* base0 = src + (q * G * T + t0) * ld + (long long)ix * bx * wy;       // member 0 of the position
        double* orow = out + s * my;
        if constexpr (MODE == DIFF_LDS) {
            for (int iy = tid; iy < my; iy += nt) mem_tot[iy] = 0.0;                        // (lane iy owns total iy throughout)
            for (int g = 0; g < G; ++g) {
                const float2* base = base0 + g * member_step;
                const double w = weights.w[g];           // (wave-uniform: a scalar load from the kernel arguments)
                for (int c0 = 0; c0 < wy; c0 += nt * PXL) {
                    const int y = c0 + tid * PXL;
                    const bool live = y < wy;                    // VEC: wy is even, so y + 1 < wy as well
                    double d0, d1;
                    strip_columns<VEC>(base, y, live, rows, bx, wy, frame_step, d0, d1);
                    if (live) stage_columns<VEC>(mem_col + y, d0, d1);
                }
                __syncthreads();
                for (int iy = tid; iy < my; iy += nt) mem_tot[iy] = member_add(mem_tot[iy], w, bin_sum_lds(mem_col, iy, by));
                __syncthreads();                                 // the next member overwrites the column sums
            }
            for (int iy = tid; iy < my; iy += nt) put_bin<ACC>(orow + iy, mem_tot[iy]);
        } else {
            for (int c0 = 0; c0 < wy; c0 += nt * PXL) {         // (wave-uniform bounds: every lane takes part in the exchange)
                const int y = c0 + tid * PXL;
                const bool live = y < wy;                        // VEC: wy is even, so y + 1 < wy as well
                const int lanes = by / PXL;                      // DIFF_SHFL: lanes per bin
                double t0sum = 0.0, t1sum = 0.0;                 // DIRECT: the totals of columns y, y + 1; SHFL: t0sum is the bin's
                for (int g = 0; g < G; ++g) {
                    const double w = weights.w[g];           // (wave-uniform: a scalar load from the kernel arguments)
                    double d0, d1;
                    strip_columns<VEC>(base0 + g * member_step, y, live, rows, bx, wy, frame_step, d0, d1);
                    if constexpr (MODE == DIFF_DIRECT) {
                        t0sum = member_add(t0sum, w, d0);
                        if constexpr (VEC) t1sum = member_add(t1sum, w, d1);
                    } else {
                        t0sum = member_add(t0sum, w, bin_sum_shfl<VEC>(d0, d1, lanes));     // (every lane of the bin holds the bin's sum; the first stores)
                    }
                }
                if constexpr (MODE == DIFF_DIRECT) {
                    if (live) put_columns<VEC, ACC>(orow + y, t0sum, t1sum);
                } else {
                    if (live && (tid & (lanes - 1)) == 0) put_bin<ACC>(orow + y / by, t0sum);
                }
            }
        }
    }
}

}  // namespace msl
