// PRISM (msl_smatrix_*): plane-wave S-matrix and probe synthesis.
//   S_b      = Propagate(pw_b),   pw_b[i, j] = exp(2 pi i (hx i / nx + hy j / ny))          one slice loop per beam and frame
//   c[p, b]  = (fx fy / (nx ny)) exp(2 pi i [hx (floor(nx/2)/nx + px/Lx) + hy (floor(ny/2)/ny + py/Ly)]) exp(-i chi(k_b))
//   psi_p(r) = W_p(r) sum_b c[p, b] S_b(r)                                                  one skinny complex GEMM per probe batch
// with the beams (hx, hy) the reciprocal-lattice points inside the aperture whose indices are multiples of the interpolation
// (fx, fy), and W_p the (nx/fx) x (ny/fy) periodic window centred on the pixel where the engine's own probe p peaks.  Axes, signs
// and the aperture rule are those of probe_kspace_kernel (potential.h); at f = (1, 1), W = 1 and psi_p is the multislice exit wave.
//
// plane_wave_kernel: a lane owns one pixel of one image of the probe buffer, (P, nx, pitch).  The phase hx i / nx + hy j / ny is
// reduced in integers ((hx i) mod nx is exact), summed in float64 turns and reduced again before the one float sincospif.  Image p
// takes beam b0 + min(p, count - 1): the images of a padded last chunk repeat its last beam.
// smatrix_coeff_kernel: a lane owns one c[p, b]; the phase is the ramp of probe_kspace_kernel term by term, minus chi in turns (the
// Cartesian float64 polynomial the probe kernels evaluate, aberration.h), reduced to one turn in float64 before the one float
// sincospif.
// smatrix_synth_kernel<G, VEC>: a workgroup of 256 lanes owns a tile of 8 rows x 32 lanes of absolute pixels (VEC: a lane owns the
// column pair, 16-byte accesses -- ny and the work pitch even; else one pixel, 8-byte accesses) and a group of G probes.  A lane
// holds G complex fp32 accumulators per pixel and walks the beams in index order: one load of S_b per beam, shared by the G probes,
// times c[p, b] read as an LDS broadcast from a chunk of SM_BEAM_CHUNK beams staged per round.  Membership in W_p is tested once per
// (probe, pixel), before the beam loop; a lane inside no window of the group loads nothing, and a tile no probe of the group touches
// stores its zeros and leaves before the beam loop.  The group index is the fastest grid dimension: the workgroups that share a
// tile of S run next to each other.  Output: the waves in natural (image, nx, pitch) order, zeros outside the window, stored to
// two buffers (the exit waves that stay, and the copy the spectrum transform consumes).  64-bit indexing; pad pixels are neither
// read nor written; no atomics: repeated calls are bitwise equal.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "aberration.h"
#include "potential.h"

namespace msl {

constexpr int SM_BEAM_CHUNK = 32;       // beams of c staged in LDS per round
constexpr int SM_TILE_ROWS = 8, SM_TILE_LANES = 32;

// psi0[p][i][j] = exp(2 pi i (hx i / nx + hy j / ny)), (hx, hy) = beams[b0 + min(p, count - 1)]
__global__ void __launch_bounds__(256) plane_wave_kernel(float2* __restrict__ psi0, const int2* __restrict__ beams, int b0, int count, int P,
                                                         int nx, int ny, int pitch) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long npix = (long long)nx * ny;
    if (i >= npix * P) return;
    const int p = (int)(i / npix);
    const long long q = i - (long long)p * npix;
    const int mx = (int)(q / ny), my = (int)(q - (long long)mx * ny);
    const int2 hb = beams[b0 + (p < count ? p : count - 1)];
    const long long rx = ((long long)hb.x * mx) % nx, ry = ((long long)hb.y * my) % ny;
    double t = (double)rx / nx + (double)ry / ny;
    t -= rint(t);
    float sn, cs;
    sincospif((float)(2.0 * t), &sn, &cs);
    psi0[((long long)p * nx + mx) * pitch + my] = make_float2(cs, sn);
}

// c[p][b], (P, Bm) complex64; scale = fx fy / (nx ny)
__global__ void __launch_bounds__(256) smatrix_coeff_kernel(float2* __restrict__ c, const double* __restrict__ xy, const int2* __restrict__ beams,
                                                            int P, int Bm, int nx, int ny, double inv_lx, double inv_ly, double kfreq_x,
                                                            double kfreq_y, double wavelength, float scale, int has_chi, ProbeAberrations ab) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long long)P * Bm) return;
    const int p = (int)(i / Bm), b = (int)(i - (long long)p * Bm);
    const int fx = beams[b].x, fy = beams[b].y;
    double t = fx * ((double)(nx / 2) / nx + xy[2 * p] * inv_lx) + fy * ((double)(ny / 2) / ny + xy[2 * p + 1] * inv_ly);
    if (has_chi) {
        const double kx = fx * kfreq_x, ky = fy * kfreq_y;       // fftfreq value = index * (1/(n*d))
        t -= aberration_chi_turns(wavelength * kx, wavelength * ky, ab, ab.a[0]);
    }
    t -= rint(t);
    float sn, cs;
    sincospif((float)(2.0 * t), &sn, &cs);
    c[i] = make_float2(scale * cs, scale * sn);
}

// first pixel of the window of probe position p along an axis of n pixels of size d: the probe peaks at (-floor(n/2) - rint(p/d)) mod n
__device__ __forceinline__ int smatrix_window_centre(int n, double d, double p) {
    long long v = (-(long long)(n / 2) - (long long)rint(p / d)) % n;
    return (int)(v < 0 ? v + n : v);
}

// is pixel i inside the periodic window of w pixels centred on c?  i, c in [0, n), w <= n
__device__ __forceinline__ bool smatrix_inside(int i, int c, int w, int n) {
    int v = i - c + w / 2;
    if (v < 0) v += n;
    if (v >= n) v -= n;
    return v < w;
}

// S: (Bm, nx, ny) dense; c: (P, Bm); out / out2: (P, nx, pitch).  grid = (ceil(P / G), ceil(nx / 8), ceil(ny / PXL / 32))
template <int G, bool VEC>
__global__ void __launch_bounds__(256) smatrix_synth_kernel(const float2* __restrict__ S, const float2* __restrict__ c, const double* __restrict__ xy,
                                                            int P, int Bm, int nx, int ny, int pitch, int win_x, int win_y, double dx, double dy,
                                                            float2* __restrict__ out, float2* __restrict__ out2) {
    constexpr int PXL = VEC ? 2 : 1;
    __shared__ float2 s_c[SM_BEAM_CHUNK][G];
    __shared__ int s_cx[G], s_cy[G];
    const int tid = threadIdx.x;
    const int p0 = blockIdx.x * G;
    const int row = blockIdx.y * SM_TILE_ROWS + tid / SM_TILE_LANES;
    const int col = (blockIdx.z * SM_TILE_LANES + tid % SM_TILE_LANES) * PXL;
    const bool valid = row < nx && col < ny;            // (VEC: ny is even, the pair is inside with its first pixel)
    if (tid < G) {
        const int p = p0 + tid;
        s_cx[tid] = p < P ? smatrix_window_centre(nx, dx, xy[2 * p]) : -1;
        s_cy[tid] = p < P ? smatrix_window_centre(ny, dy, xy[2 * p + 1]) : -1;
    }
    __syncthreads();
    unsigned m0 = 0, m1 = 0;                            // bit g: the lane's first / second pixel is inside the window of probe p0 + g
    if (valid) {
#pragma unroll
        for (int g = 0; g < G; ++g) {
            if (s_cx[g] < 0) continue;
            const bool in_x = smatrix_inside(row, s_cx[g], win_x, nx);
            if (in_x && smatrix_inside(col, s_cy[g], win_y, ny)) m0 |= 1u << g;
            if (VEC && in_x && smatrix_inside(col + 1, s_cy[g], win_y, ny)) m1 |= 1u << g;
        }
    }
    const bool active = (m0 | m1) != 0;
    const bool tile_active = __syncthreads_or(active) != 0;
    float2 a0[G], a1[G];
#pragma unroll
    for (int g = 0; g < G; ++g) { a0[g] = make_float2(0.f, 0.f); a1[g] = make_float2(0.f, 0.f); }
    if (tile_active) {
        const float2* s_px = S + (long long)row * ny + col;
        const long long beam_stride = (long long)nx * ny;
        for (int bc0 = 0; bc0 < Bm; bc0 += SM_BEAM_CHUNK) {
            __syncthreads();
            for (int idx = tid; idx < SM_BEAM_CHUNK * G; idx += 256) {
                const int g = idx / SM_BEAM_CHUNK, bb = idx - g * SM_BEAM_CHUNK;
                const int p = p0 + g, b = bc0 + bb;
                s_c[bb][g] = (p < P && b < Bm) ? c[(long long)p * Bm + b] : make_float2(0.f, 0.f);
            }
            __syncthreads();
            if (!active) continue;
            const int nb = Bm - bc0 < SM_BEAM_CHUNK ? Bm - bc0 : SM_BEAM_CHUNK;
#pragma unroll 4
            for (int bb = 0; bb < nb; ++bb) {
                const float2* sp = s_px + (long long)(bc0 + bb) * beam_stride;
                float2 v0, v1 = make_float2(0.f, 0.f);
                if constexpr (VEC) {
                    const float4 v = *reinterpret_cast<const float4*>(sp);
                    v0 = make_float2(v.x, v.y); v1 = make_float2(v.z, v.w);
                } else {
                    v0 = *sp;
                }
#pragma unroll
                for (int g = 0; g < G; ++g) {
                    const float2 w = s_c[bb][g];
                    a0[g].x = fmaf(w.x, v0.x, a0[g].x); a0[g].x = fmaf(-w.y, v0.y, a0[g].x);
                    a0[g].y = fmaf(w.x, v0.y, a0[g].y); a0[g].y = fmaf(w.y, v0.x, a0[g].y);
                    if constexpr (VEC) {
                        a1[g].x = fmaf(w.x, v1.x, a1[g].x); a1[g].x = fmaf(-w.y, v1.y, a1[g].x);
                        a1[g].y = fmaf(w.x, v1.y, a1[g].y); a1[g].y = fmaf(w.y, v1.x, a1[g].y);
                    }
                }
            }
        }
    }
    if (!valid) return;
#pragma unroll
    for (int g = 0; g < G; ++g) {
        if (p0 + g >= P) break;
        const bool i0 = (m0 >> g) & 1u, i1 = (m1 >> g) & 1u;
        const long long o = ((long long)(p0 + g) * nx + row) * pitch + col;
        if constexpr (VEC) {
            const float4 v = make_float4(i0 ? a0[g].x : 0.f, i0 ? a0[g].y : 0.f, i1 ? a1[g].x : 0.f, i1 ? a1[g].y : 0.f);
            *reinterpret_cast<float4*>(out + o) = v;
            *reinterpret_cast<float4*>(out2 + o) = v;
        } else {
            const float2 v = make_float2(i0 ? a0[g].x : 0.f, i0 ? a0[g].y : 0.f);
            out[o] = v;
            out2[o] = v;
        }
    }
}

// The cropped synthesis (msl_smatrix_probes_cropped): the window of probe p is wx = nx/fx consecutive pixels modulo nx and wx divides
// nx, so i -> i mod wx maps it one-to-one onto [0, wx) (likewise y).  The folded wave psi_c[i mod wx, j mod wy] = psi_p[i, j], (i, j)
// inside W_p, has fft2(psi_c)[m, n] = fft2(psi_p)[fx m, fy n] exactly, with no phase ramp: exp(-2 pi i m (i mod wx) / wx) =
// exp(-2 pi i (fx m) i / nx).  Tiling, probe groups, the LDS chunks of c, the beam order and the membership test are those of
// smatrix_synth_kernel, over the same absolute pixels; the value of probe p at absolute pixel (row, col) is stored at
// ((p wx + row mod wx) pitch_c + col mod wy) of the two outputs, (P, wx, pitch_c).  Nothing is stored for a pixel outside the window,
// and a tile no window of the group touches leaves before any load or store: every cropped pixel is written exactly once (no zero
// fill), pad pixels are neither read nor written.  VEC (16-byte accesses) needs ny, wy and pitch_c even: col even then implies
// col mod wy even, and the pair stays adjacent and aligned; a pair the window edge cuts stores its inside pixel alone (the other
// slot belongs to the pixel wy columns away).  64-bit indexing; no atomics: repeated calls are bitwise equal.
// S: (Bm, nx, ny) dense; c: (P, Bm); out / out2: (P, win_x, pitch_c).  grid = (ceil(P / G), ceil(nx / 8), ceil(ny / PXL / 32))
template <int G, bool VEC>
__global__ void __launch_bounds__(256) smatrix_synth_crop_kernel(const float2* __restrict__ S, const float2* __restrict__ c, const double* __restrict__ xy,
                                                                 int P, int Bm, int nx, int ny, int pitch_c, int win_x, int win_y, double dx, double dy,
                                                                 float2* __restrict__ out, float2* __restrict__ out2) {
    constexpr int PXL = VEC ? 2 : 1;
    __shared__ float2 s_c[SM_BEAM_CHUNK][G];
    __shared__ int s_cx[G], s_cy[G];
    const int tid = threadIdx.x;
    const int p0 = blockIdx.x * G;
    const int row = blockIdx.y * SM_TILE_ROWS + tid / SM_TILE_LANES;
    const int col = (blockIdx.z * SM_TILE_LANES + tid % SM_TILE_LANES) * PXL;
    const bool valid = row < nx && col < ny;            // (VEC: ny is even, the pair is inside with its first pixel)
    if (tid < G) {
        const int p = p0 + tid;
        s_cx[tid] = p < P ? smatrix_window_centre(nx, dx, xy[2 * p]) : -1;
        s_cy[tid] = p < P ? smatrix_window_centre(ny, dy, xy[2 * p + 1]) : -1;
    }
    __syncthreads();
    unsigned m0 = 0, m1 = 0;                            // bit g: the lane's first / second pixel is inside the window of probe p0 + g
    if (valid) {
#pragma unroll
        for (int g = 0; g < G; ++g) {
            if (s_cx[g] < 0) continue;
            const bool in_x = smatrix_inside(row, s_cx[g], win_x, nx);
            if (in_x && smatrix_inside(col, s_cy[g], win_y, ny)) m0 |= 1u << g;
            if (VEC && in_x && smatrix_inside(col + 1, s_cy[g], win_y, ny)) m1 |= 1u << g;
        }
    }
    const bool active = (m0 | m1) != 0;
    if (__syncthreads_or(active) == 0) return;          // (uniform over the workgroup) no window of the group touches the tile
    float2 a0[G], a1[G];
#pragma unroll
    for (int g = 0; g < G; ++g) { a0[g] = make_float2(0.f, 0.f); a1[g] = make_float2(0.f, 0.f); }
    const float2* s_px = S + (long long)row * ny + col;
    const long long beam_stride = (long long)nx * ny;
    for (int bc0 = 0; bc0 < Bm; bc0 += SM_BEAM_CHUNK) {
        __syncthreads();
        for (int idx = tid; idx < SM_BEAM_CHUNK * G; idx += 256) {
            const int g = idx / SM_BEAM_CHUNK, bb = idx - g * SM_BEAM_CHUNK;
            const int p = p0 + g, b = bc0 + bb;
            s_c[bb][g] = (p < P && b < Bm) ? c[(long long)p * Bm + b] : make_float2(0.f, 0.f);
        }
        __syncthreads();
        if (!active) continue;
        const int nb = Bm - bc0 < SM_BEAM_CHUNK ? Bm - bc0 : SM_BEAM_CHUNK;
#pragma unroll 4
        for (int bb = 0; bb < nb; ++bb) {
            const float2* sp = s_px + (long long)(bc0 + bb) * beam_stride;
            float2 v0, v1 = make_float2(0.f, 0.f);
            if constexpr (VEC) {
                const float4 v = *reinterpret_cast<const float4*>(sp);
                v0 = make_float2(v.x, v.y); v1 = make_float2(v.z, v.w);
            } else {
                v0 = *sp;
            }
#pragma unroll
            for (int g = 0; g < G; ++g) {
                const float2 w = s_c[bb][g];
                a0[g].x = fmaf(w.x, v0.x, a0[g].x); a0[g].x = fmaf(-w.y, v0.y, a0[g].x);
                a0[g].y = fmaf(w.x, v0.y, a0[g].y); a0[g].y = fmaf(w.y, v0.x, a0[g].y);
                if constexpr (VEC) {
                    a1[g].x = fmaf(w.x, v1.x, a1[g].x); a1[g].x = fmaf(-w.y, v1.y, a1[g].x);
                    a1[g].y = fmaf(w.x, v1.y, a1[g].y); a1[g].y = fmaf(w.y, v1.x, a1[g].y);
                }
            }
        }
    }
    if (!active) return;
    // (row mod wx, col mod wy) of the lane's first pixel; VEC: col and wy even, so the second pixel is the next one of the same row
    const long long o_lane = (long long)(row % win_x) * pitch_c + col % win_y;
#pragma unroll
    for (int g = 0; g < G; ++g) {
        const bool i0 = (m0 >> g) & 1u, i1 = (m1 >> g) & 1u;
        if (!(i0 || i1)) continue;                      // (a probe past P has no bit)
        const long long o = (long long)(p0 + g) * win_x * pitch_c + o_lane;
        if constexpr (VEC) {
            if (i0 && i1) {
                const float4 v = make_float4(a0[g].x, a0[g].y, a1[g].x, a1[g].y);
                *reinterpret_cast<float4*>(out + o) = v;
                *reinterpret_cast<float4*>(out2 + o) = v;
            } else if (i0) {
                out[o] = a0[g]; out2[o] = a0[g];
            } else {
                out[o + 1] = a1[g]; out2[o + 1] = a1[g];
            }
        } else {
            out[o] = a0[g];
            out2[o] = a0[g];
        }
    }
}

}  // namespace msl
