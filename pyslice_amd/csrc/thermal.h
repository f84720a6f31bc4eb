// Frozen phonons (Einstein model): the positions of a group of configurations, generated on the device from one resident base
// structure (msl_set_structure / msl_build_thermal, include/mslice.h).  The definition is pyslice_amd/thermal.py:
//   counter of atom i, configuration c: (i, c & 0xffffffff, c >> 32, 0)      key: (seed & 0xffffffff, seed >> 32)
//   x0..x3 = Philox-4x32-10 (Salmon et al., SC'11; Random123)                u_j = (x_j + 0.5) 2^-32 in (0, 1)
//   g_x = sqrt(-2 ln u0) cos(2 pi u1)   g_y = sqrt(-2 ln u0) sin(2 pi u1)    g_z = sqrt(-2 ln u2) cos(2 pi u3)
//   pos = pos0 + sigma (g_x, g_y, g_z)     in columns 0, 1, 2 of the positions, whatever the slice axis is
// A configuration is a pure function of (seed, c, i): nothing per configuration is stored or crosses PCIe, and any configuration
// can be made again at any time (the rebuilds per probe batch of the calculator's split loop are regenerations by index).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace msl {

// Philox-4x32, 10 rounds: multipliers 0xD2511F53 / 0xCD9E8D57, the key advances by the Weyl constants 0x9E3779B9 / 0xBB67AE85
__device__ __forceinline__ void philox4x32_10(uint32_t (&c)[4], uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c[0], p1 = (uint64_t)0xCD9E8D57u * c[2];       // 32 x 32 -> 64 bits
        const uint32_t hi0 = (uint32_t)(p0 >> 32), lo0 = (uint32_t)p0, hi1 = (uint32_t)(p1 >> 32), lo1 = (uint32_t)p1;
        c[0] = hi1 ^ c[1] ^ k0; c[1] = lo1;
        c[2] = hi0 ^ c[3] ^ k1; c[3] = lo0;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
}

// One thread per (configuration of the group, atom): a = f * n + i writes row a of `pos`, the frame-major (n_configs, n, 3) layout
// that stage_atoms copies into and atom_prep_kernel reads.  Box-Muller in double: (x + 0.5) 2^-32 is exact, u > 0 keeps the
// logarithm finite (|g| <= sqrt(66 ln 2) < 6.77).  The product and the sum round separately, as the definition's NumPy does, and
// sigma = 0 leaves pos0 as it is, bit for bit.
__global__ void __launch_bounds__(256) thermal_positions_kernel(const double* __restrict__ pos0, const double* __restrict__ sigma,
                                                                long long n, int n_configs, unsigned long long seed,
                                                                unsigned long long first_config, double* __restrict__ pos) {
#pragma clang fp contract(off)
    const long long a = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (a >= n * n_configs) return;
    const int f = (int)(a / n);
    const long long i = a - (long long)f * n;
    const unsigned long long cfg = first_config + (unsigned long long)f;
    uint32_t x[4] = {(uint32_t)i, (uint32_t)cfg, (uint32_t)(cfg >> 32), 0u};
    philox4x32_10(x, (uint32_t)seed, (uint32_t)(seed >> 32));
    const double scale = 1.0 / 4294967296.0;
    const double u0 = ((double)x[0] + 0.5) * scale, u1 = ((double)x[1] + 0.5) * scale;
    const double u2 = ((double)x[2] + 0.5) * scale, u3 = ((double)x[3] + 0.5) * scale;
    const double r01 = sqrt(-2.0 * log(u0)), r23 = sqrt(-2.0 * log(u2));
    double s01, c01, s23, c23;
    sincospi(2.0 * u1, &s01, &c01);
    sincospi(2.0 * u3, &s23, &c23);
    (void)s23;
    const double sg = sigma[i];
    const double gx = sg * (r01 * c01), gy = sg * (r01 * s01), gz = sg * (r23 * c23);
    pos[a * 3 + 0] = pos0[i * 3 + 0] + gx;
    pos[a * 3 + 1] = pos0[i * 3 + 1] + gy;
    pos[a * 3 + 2] = pos0[i * 3 + 2] + gz;
}

}  // namespace msl
