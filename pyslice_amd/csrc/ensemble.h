// Ensembles of member probes per scan position (partial coherence of the probe; the definition is pyslice_amd/coherence.py).
// Position q of a scan is G waves of the batch, b = q * G + g, member g built at its own offset and defocus and weighted w_g.
//
// probe_kspace_member_kernel (msl_set_probe_members): probe_kspace_aberr_kernel with the C10 coefficient of the polynomial taken per
//   probe from a device array, a0[p] = (C10 + defocus[p]) / (2 lambda); every other term, the aperture rule, the ramp and the
//   reduction of the phase to one turn in float64 before the one float sincospif are those of that kernel.
//
// diffract_members_kernel (msl_diffract_members, msl_dose_add_members): diffract_kernel's pattern pass with the G members of a
//   position folded on the device,
//     out[(q * mx + ix) * my + iy] = sum_{g < G} w_g * D[q * G + g, ix, iy],      D = msl_diffract's result for that wave.
//   Strip-major like diffract_kernel, a strip being one row of bins of one POSITION: the workgroup walks the G members of the strip
//   in order and forms, per member, the column sums exactly as diffract_kernel does (16-byte loads where ld, wy and the base allow,
//   else 8-byte loads; fp32 partial sums of at most DIFF_ROWS addends; float64 from there on) and the bin sums in the same three
//   modes with the same owner lane; the owner then adds w_g * that sum to the bin's float64 total -- one rounded multiply and one
//   rounded add, never contracted, so the result is bit for bit the host's float64 sum of w_g * D_g in member order.  Every complex
//   value is read once, 1 / G of msl_diffract's output is written, no atomics.  ACC adds the totals to out (msl_dose_add_members).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>

#include "diffract.h"
#include "potential.h"

namespace msl {

constexpr int MEMBERS_MAX = 128;                // include/mslice.h: MSL_MEMBERS_MAX

// the member weights, passed to the kernel by value (1 KB of kernel arguments: no upload, nothing of the caller's read after the launch)
struct MemberWeights {
    double w[MEMBERS_MAX];
};

__global__ void probe_kspace_member_kernel(float2* __restrict__ psik, const double* __restrict__ xy, const double* __restrict__ a0, int P,
                                           int nx, int ny, int pitch, double inv_lx, double inv_ly, double kfreq_x, double kfreq_y,
                                           double radius, double wavelength, ProbeAberrations ab) {
    long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    long long npix = (long long)nx * ny;
    if (i >= npix * P) return;
    int p = (int)(i / npix);
    long long q = i - (long long)p * npix;
    int mx = (int)(q / ny), my = (int)(q - (long long)mx * ny);
    const long long o = ((long long)p * nx + mx) * pitch + my;
    int fx = signed_freq(mx, nx), fy = signed_freq(my, ny);
    double kx = fx * kfreq_x, ky = fy * kfreq_y;       // fftfreq value = index * (1/(n*d))
    bool inside = sqrt(kx * kx + ky * ky) < radius;
    if (!inside) { psik[o] = make_float2(0.f, 0.f); return; }
    double t = fx * ((double)(nx / 2) / nx + xy[2 * p] * inv_lx) + fy * ((double)(ny / 2) / ny + xy[2 * p + 1] * inv_ly);
    const double ax = wavelength * kx, ay = wavelength * ky;
    const double r2 = fma(ax, ax, ay * ay);
    // z^m = (ax + i ay)^m, m = 2 .. 6
    const double c2 = fma(ax, ax, -ay * ay), s2 = 2.0 * ax * ay;
    const double c3 = fma(c2, ax, -s2 * ay), s3 = fma(c2, ay, s2 * ax);
    const double c4 = fma(c3, ax, -s3 * ay), s4 = fma(c3, ay, s3 * ax);
    const double c5 = fma(c4, ax, -s4 * ay), s5 = fma(c4, ay, s4 * ax);
    const double c6 = fma(c5, ax, -s5 * ay), s6 = fma(c5, ay, s5 * ax);
    // radial factors, Horner in alpha^2, as probe_kspace_aberr_kernel; the C10 coefficient is the probe's own
    double chi = r2 * fma(r2, fma(r2, ab.a[10], ab.a[4]), a0[p]);
    chi = fma(ax, r2 * fma(r2, ab.a[7], ab.a[2]), chi);
    chi = fma(ay, r2 * fma(r2, ab.b[7], ab.b[2]), chi);
    chi = fma(c2, fma(r2, fma(r2, ab.a[11], ab.a[5]), ab.a[1]), chi);
    chi = fma(s2, fma(r2, fma(r2, ab.b[11], ab.b[5]), ab.b[1]), chi);
    chi = fma(c3, fma(r2, ab.a[8], ab.a[3]), chi);
    chi = fma(s3, fma(r2, ab.b[8], ab.b[3]), chi);
    chi = fma(c4, fma(r2, ab.a[12], ab.a[6]), chi);
    chi = fma(s4, fma(r2, ab.b[12], ab.b[6]), chi);
    chi = fma(c5, ab.a[9], chi);
    chi = fma(s5, ab.b[9], chi);
    chi = fma(c6, ab.a[13], chi);
    chi = fma(s6, ab.b[13], chi);
    t -= chi;
    t -= rint(t);
    float sn, cs;
    sincospif((float)(2.0 * t), &sn, &cs);
    psik[o] = make_float2(cs, sn);
}

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
    // the column sums of the strip at `base` for this lane's columns y (and y + 1): diffract_kernel's walk over the rows.
    // KEEP THIS BODY TEXTUALLY IDENTICAL to the `batch` lambda and the row loop of diffract_kernel (diffract.h): the bitwise statements
    // of this file (the fold equals the host's fold of msl_diffract's output; G = 1, w = 1 is msl_diffract) need the fp32 sums
    // f0 += x * x + y * y to be formed -- and contracted into fused multiply-adds -- the same way in both kernels, and only the float64
    // weighted add below is pinned by a pragma.  tests/test_gpu_coherence.py compares the two kernels bit for bit in every variant: an
    // edit of one body without the other, or a compiler that contracts the two copies differently, fails there.
    auto columns = [&](const float2* base, int y, bool live, double& d0, double& d1) {
        d0 = 0.0; d1 = 0.0;
        long long off = 0;                                       // wave-uniform: offset of row r of the strip
        int a = 0;
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
    };
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
                    columns(base, y, live, d0, d1);
                    if (live) {
                        mem_col[y] = d0;
                        if constexpr (VEC) mem_col[y + 1] = d1;
                    }
                }
                __syncthreads();
                for (int iy = tid; iy < my; iy += nt) {
                    const double* c = mem_col + iy * by;
                    double v = 0.0;
                    for (int i = 0; i < by; ++i) v += c[i];
                    mem_tot[iy] = member_add(mem_tot[iy], w, v);
                }
                __syncthreads();                                 // the next member overwrites the column sums
            }
            for (int iy = tid; iy < my; iy += nt) {
                if constexpr (ACC) orow[iy] += mem_tot[iy];
                else orow[iy] = mem_tot[iy];
            }
        } else {
            for (int c0 = 0; c0 < wy; c0 += nt * PXL) {         // (wave-uniform bounds: every lane takes part in the exchange)
                const int y = c0 + tid * PXL;
                const bool live = y < wy;                        // VEC: wy is even, so y + 1 < wy as well
                double t0sum = 0.0, t1sum = 0.0;                 // DIRECT: the totals of columns y, y + 1; SHFL: t0sum is the bin's
                for (int g = 0; g < G; ++g) {
                    const double w = weights.w[g];           // (wave-uniform: a scalar load from the kernel arguments)
                    double d0, d1;
                    columns(base0 + g * member_step, y, live, d0, d1);
                    if constexpr (MODE == DIFF_DIRECT) {
                        t0sum = member_add(t0sum, w, d0);
                        if constexpr (VEC) t1sum = member_add(t1sum, w, d1);
                    } else {
                        const int lanes = by / PXL;              // lanes per bin: a power of two <= 64 that divides the wave
                        double v = VEC ? d0 + d1 : d0;
                        for (int o = lanes >> 1; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
                        t0sum = member_add(t0sum, w, v);         // (every lane of the bin holds the bin's sum; the first stores)
                    }
                }
                if constexpr (MODE == DIFF_DIRECT) {
                    if (live) {
                        if constexpr (ACC) {
                            orow[y] += t0sum;
                            if constexpr (VEC) orow[y + 1] += t1sum;
                        } else if constexpr (VEC) *reinterpret_cast<double2*>(orow + y) = make_double2(t0sum, t1sum);
                        else orow[y] = t0sum;
                    }
                } else {
                    const int lanes = by / PXL;
                    if (live && (tid & (lanes - 1)) == 0) {
                        if constexpr (ACC) orow[y / by] += t0sum;
                        else orow[y / by] = t0sum;
                    }
                }
            }
        }
    }
}

}  // namespace msl
