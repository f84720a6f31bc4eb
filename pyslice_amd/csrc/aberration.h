// Aberration function of a lens in Cartesian form, in the order of include/mslice.h (msl_set_aberrations):
// C10 C12 C21 C23 C30 C32 C34 C41 C43 C45 C50 C52 C54 C56.  With alpha = lambda k and z = alpha_x + i alpha_y
//   chi / (2 pi) = sum_nm (alpha^2)^((n+1-m)/2) (a_nm Re z^m + b_nm Im z^m),   (a_nm, b_nm) = C_nm (cos, sin)(m phi_nm) / ((n+1) lambda)
// in turns; n + 1 - m is even for every term, so the sum is a polynomial in alpha_x, alpha_y.  The probes (potential.h), the PRISM
// coefficients (smatrix.h) and the objective lens (image.h) all evaluate the one function below, so they agree term by term.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

namespace msl {

// the coefficients, passed to a kernel by value
struct ProbeAberrations {
    double a[14], b[14];
};

// from 14 (magnitude C_nm, angle phi_nm) pairs: the polynomial below then gives chi / (2 pi) in turns
inline ProbeAberrations probe_aberrations(const double* polar14x2, double wavelength) {
    static const int term_n[14] = {1, 1, 2, 2, 3, 3, 3, 4, 4, 4, 5, 5, 5, 5}, term_m[14] = {0, 2, 1, 3, 0, 2, 4, 1, 3, 5, 0, 2, 4, 6};
    ProbeAberrations ab;
    for (int k = 0; k < 14; ++k) {
        const double w = polar14x2[2 * k] / ((term_n[k] + 1) * wavelength);
        ab.a[k] = term_m[k] ? w * cos(term_m[k] * polar14x2[2 * k + 1]) : w;
        ab.b[k] = term_m[k] ? w * sin(term_m[k] * polar14x2[2 * k + 1]) : 0.0;
    }
    return ab;
}

// alpha^2 and z^m = (ax + i ay)^m = c[m] + i s[m], m = 1 .. 6 (c[0], s[0] are not used): what the polynomial and its derivatives with
// respect to the coefficients (aberration_basis) are both made from
struct AberrationPowers {
    double r2, c[7], s[7];
};

__device__ __forceinline__ AberrationPowers aberration_powers(double ax, double ay) {
    AberrationPowers w;
    w.r2 = fma(ax, ax, ay * ay);
    w.c[0] = 1.0; w.s[0] = 0.0;
    w.c[1] = ax; w.s[1] = ay;
    w.c[2] = fma(ax, ax, -ay * ay); w.s[2] = 2.0 * ax * ay;
#pragma unroll
    for (int m = 3; m <= 6; ++m) {
        w.c[m] = fma(w.c[m - 1], ax, -w.s[m - 1] * ay);
        w.s[m] = fma(w.c[m - 1], ay, w.s[m - 1] * ax);
    }
    return w;
}

// the factors of the coefficients in chi / (2 pi): A[j] = (alpha^2)^((n+1-m)/2) Re z^m and B[j] the same with Im z^m, in the order of
// the fourteen terms (B of an m = 0 term is zero) -- d(chi / 2 pi) / da_j and / db_j
__device__ __forceinline__ void aberration_basis(const AberrationPowers& w, double (&A)[14], double (&B)[14]) {
    const double r2 = w.r2, r4 = r2 * r2;
    const double rad[14] = {r2, 1.0, r2, 1.0, r4, r2, 1.0, r4, r2, 1.0, r4 * r2, r4, r2, 1.0};
    constexpr int term_m[14] = {0, 2, 1, 3, 0, 2, 4, 1, 3, 5, 0, 2, 4, 6};
#pragma unroll
    for (int j = 0; j < 14; ++j) { A[j] = rad[j] * w.c[term_m[j]]; B[j] = rad[j] * w.s[term_m[j]]; }
}

// chi / (2 pi) in turns at alpha = (ax, ay) = lambda k.  a0 is the C10 coefficient, ab.a[0] or a probe's own (ensemble.h).  Every step
// is an explicit fma or a lone multiply: the same bits wherever it is inlined.
__device__ __forceinline__ double aberration_chi_turns(const AberrationPowers& w, double ax, double ay, const ProbeAberrations& ab, double a0) {
    const double r2 = w.r2;
    const double c2 = w.c[2], s2 = w.s[2], c3 = w.c[3], s3 = w.s[3], c4 = w.c[4], s4 = w.s[4], c5 = w.c[5], s5 = w.s[5], c6 = w.c[6], s6 = w.s[6];
    // radial factors, Horner in alpha^2: m = 0: C10 C30 C50, 1: C21 C41, 2: C12 C32 C52, 3: C23 C43, 4: C34 C54, 5: C45, 6: C56
    double chi = r2 * fma(r2, fma(r2, ab.a[10], ab.a[4]), a0);
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
    return chi;
}

__device__ __forceinline__ double aberration_chi_turns(double ax, double ay, const ProbeAberrations& ab, double a0) {
    return aberration_chi_turns(aberration_powers(ax, ay), ax, ay, ab, a0);
}

}  // namespace msl
