// Band limit (anti-aliasing) of the transmission functions (msl_set_bandlimit).
//   B_d = ifft_d m_d fft_d,   m_d[h] = 1 for |h| <= cut_d, else 0   (h = the signed FFT frequency index of an axis of n_d points)
// Every slice t of a freshly built transmission stack is replaced by B_x B_y t.  The two transforms of an axis run on the generic line
// kernel (fft_generic.h: forward, x weight vector, inverse, in place, as the column step of the two-pass slice loop does with the
// Fresnel table); what this file adds is the weight vector: the mask with the 1/n of the unnormalised transform pair folded in,
// written on the device from the integer cut, so that host and device cannot disagree about a bin at the edge.
// The mask is even and separable: a transposed slice limited with the cuts swapped equals the transposed limited slice.  The host
// code (mslice.hip: bandlimit_built) limits the stack in natural order and transposes afterwards, so the result does not depend on
// the layout the slice loop keeps.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace msl {

constexpr int BL_BLOCK = 256;

// w[m] = (|f(m)| <= cut ? 1/n : 0, 0) for m < n; f = the signed frequency index (potential.h: signed_freq).  One lane per entry.
__global__ void __launch_bounds__(BL_BLOCK) bandlimit_mask_kernel(int n, int cut, float2* __restrict__ w) {
    const int m = blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= n) return;
    const int f = signed_freq(m, n);
    const bool keep = (f < 0 ? -f : f) <= cut;
    w[m] = make_float2(keep ? (float)(1.0 / (double)n) : 0.f, 0.f);
}

}  // namespace msl
