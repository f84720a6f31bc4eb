// Thickness series of the probe-batch modes (msl_set_layer_reduce): every tapped layer is reduced at
// once, inside the launch sequence of the slice loop, so that one reused block of spectra serves any number of thicknesses.
//
//   lr_layout()            host only, no device: where the results of layer l live in the float64 staging area.
//   pacbed_add_kernel      acc[l, m] += sum_{b < B} stage[l, b, m], the position-averaged pattern of every layer, in probe order.
//
// Staging, in doubles, for L = n + 1 layers of P probes x T frame slots (sections a mode does not run have no room):
//   diffract  (L, P, mx * my)    first: diffract_kernel stores column pairs with 16-byte accesses, and the base of the allocation
//                                and every layer's part of this section (P * mx * my doubles, my even whenever pairs are stored)
//                                are 16-byte aligned
//   detect    (L, P * T, D)      rows b * count + j of a sequence over `count` frame slots: the first B * count rows of a layer's part
//   polar     (L, P * T, n_bins)   are the first B probes, which is what the fetch downloads
//   pacbed    (L, mx * my)       the accumulator, last
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace msl {

enum : unsigned { LR_DETECT = 1, LR_POLAR = 2, LR_DIFFRACT = 4, LR_PACBED = 8, LR_ALL = 15 };   // include/mslice.h: MSL_LR_*

struct LrLayout {
    int64_t L = 0, P = 0, T = 0, D = 0, n_bins = 0, M = 0;                  // M = mx * my
    size_t diff_off = 0, det_off = 0, pol_off = 0, acc_off = 0, total = 0;  // doubles from the base of the staging area
    size_t diff_layer = 0, det_layer = 0, pol_layer = 0;                    // doubles per layer of each section
    size_t diff(int64_t l) const { return diff_off + (size_t)l * diff_layer; }
    size_t det(int64_t l) const { return det_off + (size_t)l * det_layer; }
    size_t pol(int64_t l) const { return pol_off + (size_t)l * pol_layer; }
    size_t acc(int64_t l) const { return acc_off + (size_t)l * (size_t)M; }
};

// false: a count below 1 where the mode needs it, or a size beyond 2^60 doubles
inline bool lr_layout(unsigned what, int64_t n_layers, int64_t P, int64_t T, int64_t D, int64_t n_bins, int64_t mx, int64_t my, LrLayout* out) {
    LrLayout y;
    if (n_layers < 1 || P < 1 || T < 1 || (what & ~LR_ALL) || !(what & LR_ALL)) return false;
    const bool patterns = what & (LR_DIFFRACT | LR_PACBED);
    if ((what & LR_DETECT) && D < 1) return false;
    if ((what & LR_POLAR) && n_bins < 1) return false;
    if (patterns && (mx < 1 || my < 1)) return false;
    const int64_t lim = (int64_t)1 << 60;
    auto mul = [&](int64_t a, int64_t b) { return (a > 0 && b > lim / a) ? (int64_t)-1 : a * b; };
    y.L = n_layers; y.P = P; y.T = T;
    y.D = (what & LR_DETECT) ? D : 0;
    y.n_bins = (what & LR_POLAR) ? n_bins : 0;
    y.M = patterns ? mul(mx, my) : 0;
    const int64_t rows = mul(P, T);
    const int64_t dl = mul(P, y.M), tl = mul(rows, y.D), pl = mul(rows, y.n_bins);
    if (rows < 0 || y.M < 0 || dl < 0 || tl < 0 || pl < 0) return false;
    const int64_t ds = mul(n_layers, dl), ts = mul(n_layers, tl), ps = mul(n_layers, pl), as = (what & LR_PACBED) ? mul(n_layers, y.M) : 0;
    if (ds < 0 || ts < 0 || ps < 0 || as < 0 || ds + ts > lim || ds + ts + ps > lim || ds + ts + ps + as > lim) return false;
    y.diff_layer = (size_t)dl; y.det_layer = (size_t)tl; y.pol_layer = (size_t)pl;
    y.diff_off = 0;
    y.det_off = (size_t)ds;
    y.pol_off = y.det_off + (size_t)ts;
    y.acc_off = y.pol_off + (size_t)ps;
    y.total = y.acc_off + (size_t)as;
    *out = y;
    return true;
}

}  // namespace msl

#ifdef __HIPCC__
#include <hip/hip_runtime.h>

namespace msl {

// acc[l * M + m] += stage[(l * P + b) * M + m] for b = 0 .. B-1, in that order, float64; blockIdx.y = layer.  One lane owns one
// pixel, or with PAIR a pair of them through 16-byte accesses (M even, both bases 16-byte aligned).  No atomics, no LDS.
template <bool PAIR>
__global__ void __launch_bounds__(256) pacbed_add_kernel(const double* __restrict__ stage, double* __restrict__ acc, int B, long long P, long long M) {
    const long long l = blockIdx.y;
    const long long m = ((long long)blockIdx.x * 256 + threadIdx.x) * (PAIR ? 2 : 1);
    if (m >= M) return;
    const double* src = stage + l * P * M + m;
    double* dst = acc + l * M + m;
    if constexpr (PAIR) {
        double2 s = *reinterpret_cast<const double2*>(dst);
        for (int b = 0; b < B; ++b) {
            const double2 v = *reinterpret_cast<const double2*>(src + (long long)b * M);
            s.x += v.x; s.y += v.y;
        }
        *reinterpret_cast<double2*>(dst) = s;
    } else {
        double s = *dst;
        for (int b = 0; b < B; ++b) s += src[(long long)b * M];
        *dst = s;
    }
}

}  // namespace msl
#endif
