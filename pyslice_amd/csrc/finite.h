// Finite projection: the part of every atom's Kirkland potential that lies IN a slice, instead of the whole
// projected atom in the one slice that holds its z.  pyslice_amd/projection.py is the float64 definition.
//
// Slabs are uniform, slab s = [e0 + s dz, e0 + (s + 1) dz); each holds J node planes at spacing h = dz / J, node n at e0 + n h.  An atom
// at z is replaced by two partial atoms on the nodes n0 = floor((z - e0) / h) and n0 + 1 with the weights 1 - w and w (total and
// z-centroid kept).  A node n reaches the 2 R + 1 slabs s with m = n - s J in [-R J, (R + 1) J); there its in-plane transform is
//     F_Z(k; alpha, beta) = sum_j a_j / (2 kappa_j^2) [S(beta, kappa_j) - S(alpha, kappa_j)] + c_j exp(-d_j k^2) 1/2 [erf(pi beta / sqrt d_j) - erf(pi alpha / sqrt d_j)]
//     kappa_j = sqrt(k^2 + b_j),  S(zeta, kappa) = sgn(zeta) (1 - exp(-2 pi kappa |zeta|)),  alpha = -m h,  beta = alpha + dz
// with alpha = -inf for the lowest slab reached (m >= R J) and beta = +inf for the highest (m < -(R - 1) J): the channels of a node
// sum to f_Z(k^2) exactly.  Channel index = species * (2 R + 1) J + (m + R J): the structure-factor kernels of potential.h take the
// channels as their "species" and the replicated rows as their atoms.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "potential.h"

namespace msl {

// S(zeta, kappa) of the header comment; zeta may be +-infinity
__device__ __forceinline__ double finite_S(double zeta, double kappa) {
    const double v = -expm1(-2.0 * M_PI * kappa * fabs(zeta));      // 1 - exp(-x) without the cancellation at small x; 1 at infinity
    return zeta < 0.0 ? -v : v;
}

// The channel tables: ff[(sp * M + mi)][kx][ky] = F_Z(k; alpha, beta) of species sp and m = mi - R J, M = (2 R + 1) J tables per species.
// float64 arithmetic, one rounding to float; one thread per (channel, kx, ky).  abcd and species as formfactor_kernel.
__global__ void finite_formfactor_kernel(float* __restrict__ ff, const double* __restrict__ abcd, const int* __restrict__ species,
                                         int n_species, int R, int J, double dz, int nx, int ny, double inv_lx, double inv_ly) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long npix = (long long)nx * ny;
    const int M = (2 * R + 1) * J;
    if (i >= npix * n_species * M) return;
    const int ch = (int)(i / npix);
    const long long p = i - (long long)ch * npix;
    const int sp = ch / M, m = ch - sp * M - R * J;
    const int mx = (int)(p / ny), my = (int)(p - (long long)mx * ny);
    const double kx = signed_freq(mx, nx) * inv_lx, ky = signed_freq(my, ny) * inv_ly;
    const double k2 = kx * kx + ky * ky;
    const double h = dz / J;
    const double alpha = (m >= R * J) ? -INFINITY : -m * h;
    const double beta = (m < -(R - 1) * J) ? INFINITY : -m * h + dz;
    const double* t = abcd + (size_t)(species[sp] - 1) * 12;
    double s1 = 0.0, s2 = 0.0;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const double kap2 = k2 + t[j * 4 + 1], kap = sqrt(kap2);
        s1 += t[j * 4 + 0] / (2.0 * kap2) * (finite_S(beta, kap) - finite_S(alpha, kap));
        const double g = M_PI / sqrt(t[j * 4 + 3]);
        s2 += t[j * 4 + 2] * exp(-t[j * 4 + 3] * k2) * 0.5 * (erf(g * beta) - erf(g * alpha));
    }
    ff[i] = (float)(s1 + s2);
}

// Per atom of a group of G frames (a = frame * n + i, as atom_prep_kernel): its rep = 2 (2 R + 1) rows, row = a * rep + j (2 R + 1) + t for
// partial atom j (node n0 + j) and the t-th slab below the highest one that node reaches.  A row has a sort key
// (frame * nz + slab) * n_channels + channel -- or -1: the atom does not count (outside [z_lo, z_hi), unknown species), the slab lies
// outside the stack, or the partial atom has no weight (w == 0: an atom on a node) --, the weight of its partial atom and the
// fractional in-plane coordinates.  e0 = lower edge of slab 0, h = node spacing.
__global__ void atom_prep_finite_kernel(const double* __restrict__ pos, const int* __restrict__ Z, long long n, int n_frames,
                                        const int* __restrict__ z_to_species, double z_lo, double z_hi, double e0, double h, int nz,
                                        int n_species, int R, int J, int ax1, int ax2, int axs, double inv_l1, double inv_l2, int* __restrict__ key,
                                        float* __restrict__ wgt, double* __restrict__ u1, double* __restrict__ u2, int* __restrict__ counts) {
    const long long a = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (a >= n * n_frames) return;
    const int frame = (int)(a / n);
    const long long i = a - (long long)frame * n;
    const int S = 2 * R + 1, M = S * J;
    const double zc = pos[a * 3 + axs];
    const int zz = Z[i];
    const int sp = (zz >= 1 && zz <= 103) ? z_to_species[zz] : -1;
    const bool counted = sp >= 0 && zc >= z_lo && zc < z_hi;
    const double g = (zc - e0) / h;
    const double gf = floor(g);
    const double w = g - gf;
    const long long n0 = counted ? (long long)gf : 0;          // (z_lo <= zc < z_hi bounds g: it fits)
    const double v1 = pos[a * 3 + ax1] * inv_l1, v2 = pos[a * 3 + ax2] * inv_l2;
    for (int j = 0; j < 2; ++j) {
        const long long node = n0 + j;
        const double wj = j ? w : 1.0 - w;
        // highest slab the node reaches: floor((node + R J) / J), floor division for negative nodes too
        const long long q = node + (long long)R * J;
        const long long s_hi = (q >= 0) ? q / J : -((-q + J - 1) / J);
        for (int t = 0; t < S; ++t) {
            const long long s = s_hi - t;
            const int m = (int)(node - s * J);                 // in [-R J, (R + 1) J)
            const bool on = counted && wj > 0.0 && s >= 0 && s < nz;
            const int k = on ? (frame * nz + (int)s) * (n_species * M) + sp * M + (m + R * J) : -1;
            const long long row = a * (2 * S) + j * S + t;
            key[row] = k;
            wgt[row] = (float)wj;
            u1[row] = v1;
            u2[row] = v2;
            if (k >= 0) atomicAdd(&counts[k], 1);
        }
    }
}

// phase_table_kernel with a real weight per row: table[i][m] = wgt[order[i]] exp(-2 pi i f(m) u[order[i]]).  A real weight keeps the table
// conjugate-symmetric, so the quadrant and mirror logic of store_quad_bin holds.  One of the two axes carries the weight.
__global__ void phase_table_weighted_kernel(float2* __restrict__ table, const double* __restrict__ u, const float* __restrict__ wgt,
                                            const int* __restrict__ order, const int* __restrict__ n_sorted_ptr, int n, int n_cols, int pitch) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long total = (long long)(*n_sorted_ptr) * n_cols;
    if (i >= total) return;
    const int a = (int)(i / n_cols), m = (int)(i - (long long)a * n_cols);
    const int src = order[a];
    if (src < 0) { table[(long long)a * pitch + m] = make_float2(0.f, 0.f); return; }       // padding row of a bin
    double t = (double)signed_freq(m, n) * u[src];
    t -= rint(t);
    float sn, cs;
    sincospif((float)(-2.0 * t), &sn, &cs);
    const float w = wgt[src];
    table[(long long)a * pitch + m] = make_float2(w * cs, w * sn);
}

}  // namespace msl
