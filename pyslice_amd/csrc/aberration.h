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

// chi / (2 pi) in turns at alpha = (ax, ay) = lambda k.  a0 is the C10 coefficient, ab.a[0] or a probe's own (ensemble.h).  Every step
// is an explicit fma or a lone multiply: the same bits wherever it is inlined.
__device__ __forceinline__ double aberration_chi_turns(double ax, double ay, const ProbeAberrations& ab, double a0) {
    const double r2 = fma(ax, ax, ay * ay);
    // z^m = (ax + i ay)^m, m = 2 .. 6
    const double c2 = fma(ax, ax, -ay * ay), s2 = 2.0 * ax * ay;
    const double c3 = fma(c2, ax, -s2 * ay), s3 = fma(c2, ay, s2 * ax);
    const double c4 = fma(c3, ax, -s3 * ay), s4 = fma(c3, ay, s3 * ax);
    const double c5 = fma(c4, ax, -s4 * ay), s5 = fma(c4, ay, s4 * ax);
    const double c6 = fma(c5, ax, -s5 * ay), s6 = fma(c5, ay, s5 * ax);
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

}  // namespace msl
