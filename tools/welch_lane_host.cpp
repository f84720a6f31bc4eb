// Host check of the per-lane arithmetic of time_welch_kernel<L> (pyslice_amd/csrc/tacaw_welch.h) for all 40 segment lengths: first-sample and
// mean removal, the fp32 window table, dif<L>, the accumulators and the digit-reversed, fftshifted store order, against a float64 Welch sum.
//   g++ -O1 -std=c++17 -o tools/bin/welch_lane_host tools/welch_lane_host.cpp && tools/bin/welch_lane_host
#include <cmath>
#include <complex>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "../pyslice_amd/csrc/fft_regs.h"
using namespace msl;
using cd = std::complex<double>;
template <int L> static double run(int T, int hop) {
    const int S = 1 + (T - L) / hop, half = L / 2;
    std::vector<std::complex<float>> x(T);
    for (int t = 0; t < T; ++t) x[t] = std::complex<float>((float)(4096.0 + 2.0 * cos(0.7 * t + 1.0) + drand48()), (float)(-1500.0 + 2.0 * sin(1.7 * t) + drand48()));
    std::vector<double> w(L); double sw2 = 0; for (int n = 0; n < L; ++n) { w[n] = 0.5 - 0.5 * cos(2 * M_PI * n / L); sw2 += w[n] * w[n]; }
    std::vector<float> g(L); std::vector<double> gd(L);
    for (int n = 0; n < L; ++n) { gd[n] = w[n] * sqrt((double)L / (S * sw2)); g[n] = (float)gd[n]; }
    float acc[L]; for (int k = 0; k < L; ++k) acc[k] = 0.f;
    std::vector<double> want(L, 0.0);
    for (int s = 0; s < S; ++s) {
        cf v[L];
        for (int k = 0; k < L; ++k) v[k] = mk(x[s * hop + k].real(), x[s * hop + k].imag());
        const cf ref = v[0];
        float sx[4] = {0, 0, 0, 0}, sy[4] = {0, 0, 0, 0};
        for (int k = 0; k < L; ++k) { v[k] = mk(v[k].x - ref.x, v[k].y - ref.y); sx[k & 3] += v[k].x; sy[k & 3] += v[k].y; }
        const float mx = ((sx[0] + sx[1]) + (sx[2] + sx[3])) * (1.f / L), my = ((sy[0] + sy[1]) + (sy[2] + sy[3])) * (1.f / L);
        for (int k = 0; k < L; ++k) v[k] = mk((v[k].x - mx) * g[k], (v[k].y - my) * g[k]);
        dif<L, 1, false, true>(v);
        for (int k = 0; k < L; ++k) acc[k] += fmaf(v[k].x, v[k].x, v[k].y * v[k].y);
        // float64 definition
        std::vector<cd> r(L); cd m = 0;
        for (int n = 0; n < L; ++n) { r[n] = cd(x[s * hop + n]) - cd(x[s * hop]); m += r[n]; }
        m /= (double)L;
        for (int f = 0; f < L; ++f) { cd a = 0; for (int n = 0; n < L; ++n) a += gd[n] * (r[n] - m) * std::polar(1.0, -2.0 * M_PI * (double)((long long)f * n % L) / L); want[f] += std::norm(a); }
    }
    want[0] = 0;
    std::vector<float> out(L, -1.f);
    for (int I = 0; I < L; ++I) { const int F = dif_out_index(I, L), KS = (F + half) % L; out[KS] = F == 0 ? 0.f : acc[I]; }
    double num = 0, den = 0;
    for (int f = 0; f < L; ++f) { const int ks = (f + half) % L; num += (out[ks] - want[f]) * (out[ks] - want[f]); den += want[f] * want[f]; }
    return sqrt(num / den);
}
int main() {
    double worst = 0;
#define X(n) { double e = run<n>(2 * n + 3, n / 2); double e2 = run<n>(n, n); if (e > worst) worst = e; if (e2 > worst) worst = e2; printf("L=%d rel-L2 %.3e  S=1: %.3e\n", n, e, e2); }
    X(16) X(18) X(20) X(24) X(25) X(27) X(30) X(32) X(36) X(40) X(45) X(48) X(50) X(54) X(60) X(64) X(72) X(75)
    X(80) X(81) X(90) X(96) X(100) X(108) X(120) X(125) X(128)
    X(21) X(28) X(35) X(42) X(49) X(56) X(63) X(70) X(84) X(98) X(105) X(112) X(126)
    printf("worst %.3e\n", worst);
    return worst < 2e-4 ? 0 : 1;
}
