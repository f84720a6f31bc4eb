// Detector response (msl_set_camera / msl_camera_frames / msl_dose_frames, include/mslice.h): the uint16 frames a camera writes for the
// electron counts of a probe batch, computed where the counts are.  The definition is pyslice_amd/camera.py (camera_frames): for pixel
// (ix, iy) of the (mx, my) pattern of probe p, c the counts as float64 and zero outside the pattern,
//   s = 0;  for a = -r .. r:  for b = -r .. r:  s = s + psf[a+r, b+r] * c[ix-a, iy-b]
//   e = gain * s;  e = e + offset;  noise > 0 only:  e = e + noise * sqrt(-2 ln u) * cos(2 pi v)
//   (u, v) = U(x0, x1), U(x2, x3) of Philox-4x32-10 (thermal.h) with the counter (ix*my + iy, p, 0, 1) under the dose's key, U = dose_uniform
//   frame = clip(rint(e), 0, full) as uint16
// camera_frames_kernel<R>: one workgroup of 256 threads owns a CAM_TX x CAM_TY = 16 x 64 tile (ix, iy) of ONE pattern of the (B, mx my)
// count staging and stages it with its halo of R in LDS, (16 + 2R) x (64 + 2R) uint32 -- 4 KiB at R = 0, 10 KiB at R = 8.  What lies
// beyond the edges of that pattern is staged as zero and never read: the patterns of a batch lie back to back, so the neighbouring
// memory is another probe's.  A wave owns 64 consecutive iy of one ix: its LDS reads of a tap are 64 consecutive words (no bank
// conflict) and its stores 128 consecutive bytes; a thread computes the 4 outputs ix = lx0 + 4 k of its column.
// R is the radius CLASS (0, 1, 2, 4, 8): msl_set_camera pads the table of a radius in between with zero weights up to its class.  A
// zero weight adds +0.0 to s (counts and weights are finite and >= 0), so the padded sum is the definition's, bit for bit, and every
// loop has a compile-time bound.  The weights are read from global memory at wave-uniform addresses (a uniform table).
// Every product and sum rounds on its own (fp contract off), in the definition's tap order: without noise the frames are the host's
// bit for bit; with noise they differ where log / sqrt / cos differ in the last place and that flips the rounding.
// Plain C++, no atomics; uint16 written with ordinary vector stores.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dose.h"
#include "thermal.h"

namespace msl {

constexpr int CAM_TX = 16;              // tile extent along ix (rows of the pattern)
constexpr int CAM_TY = 64;              // tile extent along iy (contiguous): one wave per row of the tile
constexpr int CAM_RADIUS_MAX = 8;

struct CameraArgs {
    const uint32_t* counts;             // (B, mx * my), dense
    const double* psf;                  // (2R+1)^2 weights of the radius class, row-major [a+R][b+R]
    uint16_t* frames;                   // (B, mx * my)
    int mx, my;
    int tiles_x, tiles_y;               // ceil(mx / CAM_TX), ceil(my / CAM_TY)
    double gain, offset, noise, full;   // full = 2^bits - 1
    uint32_t k0, k1, probe0;
};

template <int R>
__global__ void __launch_bounds__(256) camera_frames_kernel(CameraArgs g) {
#pragma clang fp contract(off)
    constexpr int LH = CAM_TX + 2 * R, LW = CAM_TY + 2 * R, W = 2 * R + 1;
    __shared__ uint32_t tile[LH * LW];
    const int t = threadIdx.x;
    const long long blk = blockIdx.x;
    const int per = g.tiles_x * g.tiles_y;                          // (the host keeps B * per below 2^31)
    const long long b = blk / per;
    const int rem = (int)(blk - b * per);
    const int x0 = (rem / g.tiles_y) * CAM_TX, y0 = (rem % g.tiles_y) * CAM_TY;
    const long long K = (long long)g.mx * g.my;
    const uint32_t* __restrict__ src = g.counts + b * K;
    for (int i = t; i < LH * LW; i += 256) {
        const int gx = x0 - R + i / LW, gy = y0 - R + i % LW;
        tile[i] = (gx >= 0 && gx < g.mx && gy >= 0 && gy < g.my) ? src[(long long)gx * g.my + gy] : 0u;
    }
    __syncthreads();
    const int ly = t & (CAM_TY - 1), lx0 = t / CAM_TY;
    double s[4] = {0.0, 0.0, 0.0, 0.0};
    for (int a = -R; a <= R; ++a) {
#pragma unroll
        for (int bb = -R; bb <= R; ++bb) {
            const double w = g.psf[(a + R) * W + (bb + R)];
#pragma unroll
            for (int k = 0; k < 4; ++k) s[k] = s[k] + w * (double)tile[(lx0 + 4 * k + R - a) * LW + (ly + R - bb)];
        }
    }
    const int iy = y0 + ly;
    if (iy >= g.my) return;
    uint16_t* __restrict__ dst = g.frames + b * K;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int ix = x0 + lx0 + 4 * k;
        if (ix >= g.mx) continue;
        const long long pixel = (long long)ix * g.my + iy;
        double e = g.gain * s[k];
        e = e + g.offset;
        if (g.noise > 0.0) {
            uint32_t x[4] = {(uint32_t)pixel, g.probe0 + (uint32_t)b, 0u, 1u};
            philox4x32_10(x, g.k0, g.k1);
            const double u = dose_uniform(x[0], x[1]), v = dose_uniform(x[2], x[3]);
            const double z = sqrt(-2.0 * log(u)) * cos(6.283185307179586 * v);
            e = e + g.noise * z;
        }
        double q = rint(e);
        q = q < 0.0 ? 0.0 : (q > g.full ? g.full : q);
        dst[pixel] = (uint16_t)q;
    }
}

}  // namespace msl
