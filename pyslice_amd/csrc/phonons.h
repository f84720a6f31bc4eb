// Phonon modes: the positions of a group of frames synthesised on the device from M lattice-dynamics modes and one resident base
// structure (msl_set_structure / msl_set_modes / msl_build_modes, include/mslice.h).  The definition is pyslice_amd/phonons.py:
//   normal coordinate of mode m under draw index k: Philox-4x32-10 of counter (m, k & 0xffffffff, k >> 32, 1) (word 3 = 0 is the
//   Einstein stream of thermal.h), key (seed & 0xffffffff, seed >> 32);  u_j = (x_j + 0.5) 2^-32;  g = sqrt(-ln u0) exp(2 pi i u1)
//   frame c:  dynamic: k = 0, theta = tau_m c      snapshots: k = c, theta = 0              frac(y) = y - rint(y)
//   C[c,m] = g_m(k) exp(-2 pi i frac(theta))       x = (q0 r0 + q1 r1) + q2 r2              E = exp(2 pi i frac(x))
//   pos = r_i + sum_m Re[(C[c,m] E) W[m, b_i, :]]  summed in mode order, in columns 0, 1, 2 whatever the slice axis is
// all in float64.  theta and x are rounded as the definition's NumPy rounds them (fp contract off: a fused multiply-add would move
// frac(x) by up to an ulp of x, 1e-13 cycles at |x| ~ 1e3); the products and sums behind E are written as explicit fma()s, which
// removes roundings and leaves the compiler no choice, so a frame comes out the same in whichever slot of a frame tile it is made.
// A frame is a pure function of (seed, c): nothing per frame is stored or crosses PCIe, and any frame can be made again at any time.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "thermal.h"

namespace msl {

// Frames per thread (the wide and the narrow tile) and modes per LDS chunk of mode_positions_kernel, and the largest basis whose W
// rows are staged in LDS.  The sincospi of E depends on (atom, mode) only: with 8 frames in registers its ~50 double instructions are
// shared by 8 frames of 10 each.  8 frames are 48 accumulator VGPRs; under __launch_bounds__(256, 4) the kernel takes 126 VGPRs and
// no scratch (tools/kernel_resources.sh): 4 waves per SIMD = 16 waves = 4 workgroups of 256 per CU, so a workgroup may use
// 160 KiB / 4 = 40 KiB of LDS without costing occupancy: a chunk of 32 modes is 32 x (8 x 16 B of C + 32 B of q, padded) = 5 KiB plus
// 32 x 48 B x n_basis of W, 29 KiB at n_basis = 16.  A larger basis reads its W rows from global memory (L2-resident: 48 B x n_basis
// x M in all).  A group of one or two frames (a frame batch of 1 or 2, msl_mode_positions) runs the kernel with a tile of 2 instead
// of accumulating six idle frames: 96 VGPRs, 5 waves per SIMD.  The arithmetic of a frame is the same explicit sequence in both.
constexpr int MODE_TILE = 8;
constexpr int MODE_TILE_SMALL = 2;
constexpr int MODE_CHUNK = 32;
constexpr int MODE_LDS_BASIS = 16;

inline size_t mode_positions_lds_bytes(int n_basis, int tile) {
    return (size_t)MODE_CHUNK * ((size_t)tile * sizeof(double2) + (n_basis <= MODE_LDS_BASIS ? (size_t)n_basis * 6 * sizeof(double) : 0) +
                                 4 * sizeof(double));        // (q rows padded to 4 doubles: every carve offset a multiple of 16)
}

// One thread per (frame of the group, mode): t = c * M + m writes C[c, m].  count * M < 2^31 (checked by the callers).
__global__ void __launch_bounds__(256) mode_coefficients_kernel(const double* __restrict__ tau, int M, int count, unsigned long long seed,
                                                                unsigned long long first_frame, int dynamic, double2* __restrict__ C) {
#pragma clang fp contract(off)
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= M * count) return;
    const int c = t / M, m = t - c * M;
    const unsigned long long frame = first_frame + (unsigned long long)c;
    const unsigned long long k = dynamic ? 0ull : frame;
    uint32_t x[4] = {(uint32_t)m, (uint32_t)k, (uint32_t)(k >> 32), 1u};
    philox4x32_10(x, (uint32_t)seed, (uint32_t)(seed >> 32));
    const double scale = 1.0 / 4294967296.0;
    const double u0 = ((double)x[0] + 0.5) * scale, u1 = ((double)x[1] + 0.5) * scale;
    const double amp = sqrt(-log(u0));
    double gs, gc;
    sincospi(2.0 * u1, &gs, &gc);
    const double gr = amp * gc, gi = amp * gs;
    const double theta = dynamic ? tau[m] * (double)frame : 0.0;        // frame < 2^31: exact in double
    const double fr = theta - rint(theta);
    double ps, pc;
    sincospi(2.0 * fr, &ps, &pc);                                       // the phase factor is (pc, -ps)
    C[t] = make_double2(gr * pc + gi * ps, gi * pc - gr * ps);
}

// x = (q0 r0 + q1 r1) + q2 r2, every product and every sum rounded separately
__device__ __forceinline__ double mode_phase(double q0, double q1, double q2, double r0, double r1, double r2) {
#pragma clang fp contract(off)
    const double a = q0 * r0, b = q1 * r1, c = q2 * r2;
    const double ab = a + b;
    return ab + c;
}

// One thread per atom, blockIdx.y per tile of TILE frames of the group: three double accumulators per frame in registers.  The
// modes are walked in chunks of MODE_CHUNK whose q, C (this tile's frames, zero beyond `count`) and -- W_LDS -- W rows the workgroup
// stages in LDS; per (atom, mode) one sincospi, per frame one complex product C E and three real accumulations (10 fma / mul; a
// frame beyond `count` accumulates zeros and is not stored).  Writes rows (f, i) of `pos`, the frame-major (count, n, 3) layout that
// stage_atoms copies into.  A basis atom whose W rows are zero keeps pos0 bit for bit (r + (+-0)).  Launch with
// mode_positions_lds_bytes(nb, TILE) of dynamic LDS; n >= 1.
template <bool W_LDS, int TILE>
__global__ void __launch_bounds__(256, 4) mode_positions_kernel(const double* __restrict__ pos0, const int* __restrict__ basis,
                                                             const double* __restrict__ q, const double2* __restrict__ C,
                                                             const double* __restrict__ W, long long n, int nb, int M, int count,
                                                             double* __restrict__ pos) {
#pragma clang fp contract(off)
    extern __shared__ __attribute__((aligned(16))) char mode_smem[];
    double2* sC = (double2*)mode_smem;                                              // [MODE_CHUNK][TILE]
    double* sq = (double*)(sC + MODE_CHUNK * TILE);                            // [MODE_CHUNK][4]
    double* sW = sq + MODE_CHUNK * 4;                                               // [MODE_CHUNK][nb][6] (W_LDS)
    const int f0 = blockIdx.y * TILE;
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    const bool live = i < n;
    const long long ic = live ? i : n - 1;                                          // (every thread takes part in the barriers)
    const double r0 = pos0[ic * 3 + 0], r1 = pos0[ic * 3 + 1], r2 = pos0[ic * 3 + 2];
    const int b = basis[ic];
    double acc[TILE][3];
#pragma unroll
    for (int f = 0; f < TILE; ++f) acc[f][0] = acc[f][1] = acc[f][2] = 0.0;
    for (int m0 = 0; m0 < M; m0 += MODE_CHUNK) {
        const int mc = min(MODE_CHUNK, M - m0);
        for (int t = threadIdx.x; t < mc * 3; t += 256) { const int mm = t / 3; sq[mm * 4 + (t - mm * 3)] = q[(size_t)m0 * 3 + t]; }
        for (int t = threadIdx.x; t < mc * TILE; t += 256) {
            const int mm = t / TILE, f = t - mm * TILE;
            sC[t] = f0 + f < count ? C[(size_t)(f0 + f) * M + m0 + mm] : make_double2(0.0, 0.0);
        }
        if (W_LDS) {
            const double* Wc = W + (size_t)m0 * nb * 6;
            for (int t = threadIdx.x; t < mc * nb * 6; t += 256) sW[t] = Wc[t];
        }
        __syncthreads();
        for (int mm = 0; mm < mc; ++mm) {
            const double x = mode_phase(sq[mm * 4 + 0], sq[mm * 4 + 1], sq[mm * 4 + 2], r0, r1, r2);
            double es, ec;
            sincospi(2.0 * (x - rint(x)), &es, &ec);
            const double* w = W_LDS ? sW + ((size_t)mm * nb + b) * 6 : W + ((size_t)(m0 + mm) * nb + b) * 6;
            const double w0r = w[0], w0i = w[1], w1r = w[2], w1i = w[3], w2r = w[4], w2i = w[5];
#pragma unroll
            for (int f = 0; f < TILE; ++f) {
                const double2 c = sC[mm * TILE + f];
                const double pr = fma(c.x, ec, -(c.y * es)), pi = fma(c.x, es, c.y * ec);
                acc[f][0] = fma(-pi, w0i, fma(pr, w0r, acc[f][0]));
                acc[f][1] = fma(-pi, w1i, fma(pr, w1r, acc[f][1]));
                acc[f][2] = fma(-pi, w2i, fma(pr, w2r, acc[f][2]));
            }
        }
        __syncthreads();
    }
    if (!live) return;
#pragma unroll
    for (int f = 0; f < TILE; ++f) {
        if (f0 + f >= count) break;
        double* o = pos + ((size_t)(f0 + f) * (size_t)n + (size_t)i) * 3;
        o[0] = r0 + acc[f][0]; o[1] = r1 + acc[f][1]; o[2] = r2 + acc[f][2];
    }
}

}  // namespace msl
