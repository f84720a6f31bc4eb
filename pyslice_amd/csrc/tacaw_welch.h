// Windowed, segment-averaged (Welch) TACAW spectra on the per-lane register network: time_welch_kernel<L>.
// For one pixel's line x[0..T), segment length L, hop, S = 1 + (T - L) / hop segments and a window table g[0..L):
//     r_s[n] = x[s hop + n] - x[s hop],   y_s[n] = g[n] (r_s[n] - mean_n r_s[n]),   I[f] = sum_s |FFT_L(y_s)[f]|^2,   I[0] := 0
// stored fftshifted along f as (n_images, L, npix) float32.  g = w sqrt(L / (S sum w^2)) comes from the host (float64, rounded once).
// The conventions are time_direct_kernel's (tacaw_regs.h): a lane per pixel, 256-lane workgroups, a grid-stride loop over tiles of
// 256 pixels, a ragged last tile that repeats the image's last pixel, raw buffer loads with a wave-uniform row offset, the
// digit-reversed order of dif<> absorbed by the store addresses, non-temporal stores.  New: the loop over the segments of a tile,
// the TRUE segment mean (once a window multiplies the line a constant leaks into every bin, so "any constant" no longer does; the
// first sample is still taken off first, which is exact in fp32 and leaves numbers of the size of the thermal part), the window,
// and L power accumulators per lane that are stored once, after the last segment.  Overlapping segments are plain re-loads.
#pragma once
#include <hip/hip_runtime.h>
#include "tacaw_regs.h"

namespace msl {

struct WelchJob {
    const float2* in;           // (n_images, T, npix) c64
    float* out;                 // (n_images, L, npix) f32, frequency axis fftshifted
    const float* g;             // (L) window x normalisation, read with scalar loads (wave-uniform per sample)
    long long in_image_stride;  // T * npix
    long long out_image_stride; // L * npix
    int npix, n_images, L, hop, S;
};

// Rows of the NEXT segment in flight while the current one is transformed, sized as tdir_prefetch sizes them: what fits beside the
// 2 L data registers and the L accumulators in a budget below the 512 registers of one wave per SIMD.  The budget is 400 where
// tdir_prefetch has 432: the window's scalars, the mean and the accumulate step take the difference, and the lengths with two
// radix-5 levels (multiples of 25) keep 16 more temporaries alive in the butterflies.  Every instantiation compiles without
// scratch (DESIGN.md section 4.4a has the table).
__host__ __device__ constexpr int twelch_budget(int L) { return L % 25 == 0 ? 384 : 400; }
__host__ __device__ constexpr int twelch_prefetch(int L) { return 5 * L <= twelch_budget(L) ? L : (twelch_budget(L) - 3 * L) / 2; }

template <int L>
__global__ void __launch_bounds__(256) time_welch_kernel(WelchJob job) {
    constexpr int PF = twelch_prefetch(L), half = L / 2, KH = (L + 1) / 2;
    const int tid = threadIdx.x;
    const int tiles_per_image = (job.npix + 255) / 256;
    const long long n_tiles = (long long)tiles_per_image * job.n_images;
    const long long step = gridDim.x;
    // (ragged last tile: the surplus lanes repeat the image's last pixel, as in time_direct_kernel)
    auto column = [&](long long t, const float2*& img, float*& orow, unsigned& c) {
        const int p = __builtin_amdgcn_readfirstlane((int)(t / tiles_per_image));
        const int c0 = __builtin_amdgcn_readfirstlane((int)(t % tiles_per_image) * 256);
        c = c0 + tid < job.npix ? (unsigned)(c0 + tid) : (unsigned)(job.npix - 1);
        img = job.in + (long long)p * job.in_image_stride;
        orow = job.out + (long long)p * job.out_image_stride;
    };
    // the L rows of segment s through two descriptors, rows below KH through the first: the 32-bit row offsets stay below 2^32 for
    // every image the host sends here (KH npix 8 bytes < 4 GB); the segment's first row moves the descriptor's base (SALU)
    auto segment = [&](const float2* img, int s, msl_i4v& rows, msl_i4v& rows_hi) {
        const float2* first = img + (long long)s * job.hop * job.npix;
        rows = make_raw_rsrc(first);
        rows_hi = make_raw_rsrc(first + (long long)KH * job.npix);
    };
    auto load_row = [&](const msl_i4v& rows, const msl_i4v& rows_hi, int k, unsigned c, int npix_now) {
        const msl_f2v t = k < KH ? msl_raw_buffer_load_f2(rows, (int)(8u * c), (int)(8u * (unsigned)k * (unsigned)npix_now), 2)
                                 : msl_raw_buffer_load_f2(rows_hi, (int)(8u * c), (int)(8u * (unsigned)(k - KH) * (unsigned)npix_now), 2);
        return make_float2(t.x, t.y);
    };
    // (the window table and the row offsets are the same for every segment: hidden from the compiler, which would otherwise keep
    // all of them in scalar registers across the loop and spill those through the vector file -- time_split_kernel's `hide`)
    auto hide_s = [](int x) { asm volatile("" : "+s"(x)); return x; };
    auto hide_p = [](unsigned long long p) { asm volatile("" : "+s"(p)); return p; };
    typedef float __attribute__((address_space(4))) msl_cfloat;      // constant address space: a uniform address is a scalar load
    constexpr int GCH = 16;
    long long tile = blockIdx.x;
    float2 nx[PF];
    const float2* img; float* orow; unsigned c;
    msl_i4v rows, rows_hi;
    if (tile < n_tiles) {
        column(tile, img, orow, c);
        segment(img, 0, rows, rows_hi);
#pragma unroll
        for (int k = 0; k < PF; ++k) nx[k] = load_row(rows, rows_hi, k, c, job.npix);
    }
    const unsigned long long gtab = (unsigned long long)job.g;
    for (; tile < n_tiles; tile += step) {
        float acc[L];
#pragma unroll
        for (int k = 0; k < L; ++k) acc[k] = 0.f;
        float* const out_rows = orow;
        const unsigned my_c = c;
        const float2* const my_img = img;
        for (int s = 0; s < job.S; ++s) {
            float2 v[L];
            const int npix_now = hide_s(job.npix);
#pragma unroll
            for (int k = 0; k < PF; ++k) v[k] = nx[k];
#pragma unroll
            for (int k = PF; k < L; ++k) v[k] = load_row(rows, rows_hi, k, c, npix_now);
            // the next segment: of this tile, or the first one of the workgroup's next tile
            if (s + 1 < job.S) {
                segment(my_img, s + 1, rows, rows_hi);
#pragma unroll
                for (int k = 0; k < PF; ++k) nx[k] = load_row(rows, rows_hi, k, c, npix_now);
            } else if (tile + step < n_tiles) {
                column(tile + step, img, orow, c);
                segment(img, 0, rows, rows_hi);
#pragma unroll
                for (int k = 0; k < PF; ++k) nx[k] = load_row(rows, rows_hi, k, c, npix_now);
            }
            __builtin_amdgcn_sched_barrier(0);
            const float2 ref = v[0];
            float2 sum4[4] = {make_float2(0.f, 0.f), make_float2(0.f, 0.f), make_float2(0.f, 0.f), make_float2(0.f, 0.f)};
#pragma unroll
            for (int k = 0; k < L; ++k) {
                v[k] = make_float2(v[k].x - ref.x, v[k].y - ref.y);
                sum4[k & 3].x += v[k].x; sum4[k & 3].y += v[k].y;
            }
            const float2 mean = make_float2(((sum4[0].x + sum4[1].x) + (sum4[2].x + sum4[3].x)) * (1.f / L),
                                            ((sum4[0].y + sum4[1].y) + (sum4[2].y + sum4[3].y)) * (1.f / L));
            // g through the scalar cache, GCH entries at a time: SGPR operands of the multiplies, no vector register spent on them
            const msl_cfloat* g = reinterpret_cast<const msl_cfloat*>(hide_p(gtab));
            static_for<0, (L + GCH - 1) / GCH>([&](auto cc) {
                constexpr int k0 = decltype(cc)::value * GCH, k1 = k0 + GCH < L ? k0 + GCH : L;
                float gk[GCH];
#pragma unroll
                for (int k = k0; k < k1; ++k) gk[k - k0] = g[k];
#pragma unroll
                for (int k = k0; k < k1; ++k) v[k] = make_float2((v[k].x - mean.x) * gk[k - k0], (v[k].y - mean.y) * gk[k - k0]);
                __builtin_amdgcn_sched_barrier(0);
            });
            dif<L, 1, false, true>(v);
#pragma unroll
            for (int k = 0; k < L; ++k) acc[k] += fmaf(v[k].x, v[k].x, v[k].y * v[k].y);
        }
        const int npix_out = hide_s(job.npix);
        static_for<0, L>([&](auto ic) {
            constexpr int I = decltype(ic)::value;
            constexpr int F = dif_out_index(I, L);                 // frequency held by register I
            constexpr int KS = (F + half) % L;                     // np.fft.fftshift
            const float val = (F == 0) ? 0.f : acc[I];
            __builtin_nontemporal_store(val, reinterpret_cast<float*>(reinterpret_cast<char*>(out_rows + (long long)KS * npix_out) + 4u * my_c));
        });
    }
}

// is there a kernel for segment length L?  (the lengths of time_direct_kernel)
bool time_welch_has(int L);
// launch on `stream`; false: no kernel for job.L (nothing launched).  Errors of the launch itself: hipGetLastError().
bool time_welch_launch(const WelchJob& job, int n_cus, hipStream_t stream);

}  // namespace msl
