// Element maps: channelling-weighted ionisation signal per element (pyslice_amd/ionization.py is the
// definition).  For channel e (an atomic number, a Gaussian of rms width w_e and a cross-section c_e) and slice s
//     W_e,s(r) = Re ifft2( c_e exp(-2 pi^2 w_e^2 |k|^2) sum_{i in A_e,s} exp(-2 pi i k r_i) ) / (dx dy)
//     I[p, e, s] = sum_r |psi_p,s(r)|^2 W_e,s(r) / sum_r |psi_p,0(r)|^2,      psi_p,s the wave arriving at slice s.
// W is the structure-factor sum of the potential build with a table that is non-zero for one species only (ion_table_kernel), through
// the build's own launchers.  The kernel here: that table.  The reduction of the slice loop and its finishing sum are slice_sums.h's,
// with the policy IonSums (float32 partials over the 512 pixel pairs of a tile, ion_wave_sum across the wave).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace msl {

constexpr int ION_MAX = 8;                  // channels

// tab (n_species, nx, ny) f32 on the fftfreq grid: amp exp(-2 pi^2 w^2 |k|^2) for species `sp`, zero for every other one (sp < 0: all
// zero).  amp = c dx dy: the build's inverse transform divides by dx^2 dy^2.
__global__ void ion_table_kernel(float* __restrict__ tab, int n_species, int sp, int nx, int ny, double inv_lx, double inv_ly, double w,
                                 double amp) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long npix = (long long)nx * ny;
    if (i >= npix * n_species) return;
    float v = 0.f;
    if ((int)(i / npix) == sp) {
        const long long p = i % npix;
        const int mx = (int)(p / ny), my = (int)(p - (long long)mx * ny);
        const double kx = (mx < (nx + 1) / 2 ? mx : mx - nx) * inv_lx, ky = (my < (ny + 1) / 2 ? my : my - ny) * inv_ly;
        v = (float)(amp * exp(-2.0 * M_PI * M_PI * w * w * (kx * kx + ky * ky)));
    }
    tab[i] = v;
}

}  // namespace msl
