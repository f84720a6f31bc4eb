// Diffraction pass (msl_diffract): frame-summed, detector-binned diffraction patterns of every probe in one launch.
//   out[(b * mx + ix) * my + iy] = sum_{j < count} sum_{a < bx} sum_{c < by} |Psi[b, t0 + j, (ix * bx + a) * wy + iy * by + c]|^2
// over a (B, T, K = wx * wy) complex64 array whose images start every `ld` pixels; mx = wx / bx, my = wy / by.
//
// Strip-major: a strip is one row of bins of one probe, i.e. the bx x wy pixels of `count` frames that end in the my bins
// (b, ix, :).  A workgroup owns a run of consecutive strips.  A lane owns one column pair (16-byte loads; one column with
// 8-byte loads when ld, wy or the base address is odd) of every chunk of 2 x blockDim columns and walks the count * bx rows of the
// strip DIFF_ROWS at a time: the loads of a batch are independent (their row offsets are wave-uniform), |Psi|^2 and the sum of a
// batch are fp32 (at most DIFF_ROWS addends per column, far inside the 1024 the detector pass allows itself), the sum over
// batches is float64.  Every complex value is read from HBM once, pad pixels (K <= k < ld) never.
// The by columns of a bin are then added in float64:
//   DIFF_DIRECT  by = 1: the lane stores its columns (16-byte stores for a column pair);
//   DIFF_SHFL    by a power of two <= 64: the columns of a bin sit in by / 2 (or by) neighbouring lanes of one wave -- xor
//                exchange, the bin's first lane stores;
//   DIFF_LDS     any other divisor of wy (3, 5, 7, 25 ...): column sums through LDS (wy doubles), lane iy adds bin iy in order.
// No atomics, fixed summation order in every mode: the same input gives bitwise the same output.
// ACC (msl_dose_add): every bin's sum is ADDED to out instead of stored -- a bin has one owner lane in every mode, so the adds
// of successive launches on one stream land in launch order, without atomics.
// The column walk and the bin sums are device functions of this file, shared with diffract_members_kernel (ensemble.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>

namespace msl {

constexpr int DIFF_ROWS = 8;                    // rows in flight per lane = fp32 addends per column before the float64 sum (tail: 4, 2, 1)
enum { DIFF_DIRECT = 0, DIFF_SHFL = 1, DIFF_LDS = 2 };

// The column walk both pattern kernels share (diffract_kernel here, diffract_members_kernel in ensemble.h): d0, d1 = the float64 sums
// of columns y and (VEC) y + 1 over the `rows` rows of the strip at `base`, bx rows of wy pixels per frame, frames frame_step further
// apart.  Every lane keeps the wave-uniform offsets; only live lanes load.  One body, so the fp32 sums f += x * x + y * y are formed
// -- and contracted into fused multiply-adds -- the same way for both kernels: the bitwise statements of ensemble.h rest on that.
template <bool VEC>
__device__ __forceinline__ void strip_columns(const float2* base, int y, bool live, int rows, int bx, int wy, long long frame_step, double& d0,
                                              double& d1) {
    d0 = 0.0; d1 = 0.0;
    long long off = 0;                                           // wave-uniform: offset of row r of the strip
    int a = 0;
    // N rows: offsets first (scalar), then N independent loads, then the fp32 sum of the N values of each column
    auto batch = [&](auto n_tag) {
        constexpr int N = decltype(n_tag)::value;
        long long o[N];
#pragma unroll
        for (int u = 0; u < N; ++u) {
            o[u] = off;
            off += wy;
            if (++a == bx) { a = 0; off += frame_step; }
        }
        if (!live) return;
        float f0 = 0.f, f1 = 0.f;
        if constexpr (VEC) {
            float4 v[N];
#pragma unroll
            for (int u = 0; u < N; ++u) v[u] = *reinterpret_cast<const float4*>(base + o[u] + y);
#pragma unroll
            for (int u = 0; u < N; ++u) {
                f0 += v[u].x * v[u].x + v[u].y * v[u].y;
                f1 += v[u].z * v[u].z + v[u].w * v[u].w;
            }
        } else {
            float2 v[N];
#pragma unroll
            for (int u = 0; u < N; ++u) v[u] = base[o[u] + y];
#pragma unroll
            for (int u = 0; u < N; ++u) f0 += v[u].x * v[u].x + v[u].y * v[u].y;
        }
        d0 += (double)f0;
        d1 += (double)f1;
    };
    int r = 0;
    for (; r + DIFF_ROWS <= rows; r += DIFF_ROWS) batch(std::integral_constant<int, DIFF_ROWS>{});
    if ((rows - r) & 4) batch(std::integral_constant<int, 4>{});
    if ((rows - r) & 2) batch(std::integral_constant<int, 2>{});
    if ((rows - r) & 1) batch(std::integral_constant<int, 1>{});
}

// DIFF_SHFL: the sum of a bin's columns, in every one of the bin's `lanes` lanes (a power of two <= 64 that divides the wave)
template <bool VEC>
__device__ __forceinline__ double bin_sum_shfl(double d0, double d1, int lanes) {
    double v = VEC ? d0 + d1 : d0;
    for (int o = lanes >> 1; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// DIFF_LDS: a lane's column sums into the strip's LDS row, then the sum of the by column sums of bin iy, in column order
template <bool VEC>
__device__ __forceinline__ void stage_columns(double* col, double d0, double d1) {
    col[0] = d0;
    if constexpr (VEC) col[1] = d1;
}

__device__ __forceinline__ double bin_sum_lds(const double* col, int iy, int by) {
    const double* c = col + iy * by;
    double v = 0.0;
    for (int i = 0; i < by; ++i) v += c[i];
    return v;
}

// the owner lane's store (ACC: add) of a bin, and of the columns y and (VEC) y + 1 of DIFF_DIRECT
template <bool ACC>
__device__ __forceinline__ void put_bin(double* dst, double v) {
    if constexpr (ACC) *dst += v;
    else *dst = v;
}

template <bool VEC, bool ACC>
__device__ __forceinline__ void put_columns(double* dst, double d0, double d1) {
    if constexpr (ACC) {
        dst[0] += d0;
        if constexpr (VEC) dst[1] += d1;
    } else if constexpr (VEC) *reinterpret_cast<double2*>(dst) = make_double2(d0, d1);
    else dst[0] = d0;
}

template <int MODE, bool VEC, bool ACC = false>
__global__ void __launch_bounds__(256) diffract_kernel(const float2* __restrict__ src, long long T, long long t0, int count, long long ld,
                                                       int wx, int wy, int bx, int by, long long strips, int strips_per_wg,
                                                       double* __restrict__ out) {
    extern __shared__ double diff_col[];        // DIFF_LDS: the wy column sums of the strip
    constexpr int PXL = VEC ? 2 : 1;            // columns per lane and chunk
    const int mx = wx / bx, my = wy / by;
    const int nt = blockDim.x, tid = threadIdx.x;
    const int rows = count * bx;
    const long long frame_step = ld - (long long)bx * wy;       // from behind the last row of a frame's strip to the next frame's first
    const long long s0 = (long long)blockIdx.x * strips_per_wg;
    const long long s1 = min(strips, s0 + strips_per_wg);
    for (long long s = s0; s < s1; ++s) {
        const long long b = s / mx;
        const int ix = (int)(s - b * mx);
        const float2* base = src + (b * T + t0) * ld + (long long)ix * bx * wy;
        double* orow = out + s * my;
        for (int c0 = 0; c0 < wy; c0 += nt * PXL) {             // (wave-uniform bounds: every lane takes part in the exchange)
            const int y = c0 + tid * PXL;
            const bool live = y < wy;                            // VEC: wy is even, so y + 1 < wy as well
            double d0, d1;
            strip_columns<VEC>(base, y, live, rows, bx, wy, frame_step, d0, d1);
            if constexpr (MODE == DIFF_DIRECT) {
                if (live) put_columns<VEC, ACC>(orow + y, d0, d1);
            } else if constexpr (MODE == DIFF_SHFL) {
                const int lanes = by / PXL;
                const double v = bin_sum_shfl<VEC>(d0, d1, lanes);
                if (live && (tid & (lanes - 1)) == 0) put_bin<ACC>(orow + y / by, v);
            } else {
                if (live) stage_columns<VEC>(diff_col + y, d0, d1);
            }
        }
        if constexpr (MODE == DIFF_LDS) {
            __syncthreads();
            for (int iy = tid; iy < my; iy += nt) put_bin<ACC>(orow + iy, bin_sum_lds(diff_col, iy, by));
            __syncthreads();                                     // the next strip overwrites the column sums
        }
    }
}

}  // namespace msl

