// Stand-alone check of the staging layout of the thickness series (pyslice_amd/csrc/layer_reduce.h: lr_layout), for a host sanitizer:
//   c++ -std=c++17 -g -O1 -fsanitize=address,undefined -o layer_reduce_layout_check tools/layer_reduce_layout_check.cpp && ./layer_reduce_layout_check
// A buffer of exactly `total` doubles is allocated and every element that a reduction of layer l writes, or that the fetch of the
// first B probes reads, is touched through the layout's offsets: one element out of bounds is an error under the sanitizer, and an
// element written twice or never is an error here.  Needs no device.
#include <cstdint>
#include <cstdio>
#include <memory>

#include "../pyslice_amd/csrc/layer_reduce.h"

static int failures = 0;

static void check(unsigned what, int64_t L, int64_t P, int64_t T, int64_t D, int64_t nb, int64_t mx, int64_t my) {
    msl::LrLayout y;
    bool good = msl::lr_layout(what, L, P, T, D, nb, mx, my, &y);
    if (good) {
        const bool det = what & msl::LR_DETECT, pol = what & msl::LR_POLAR, pat = what & (msl::LR_DIFFRACT | msl::LR_PACBED);
        const int64_t M = pat ? mx * my : 0;
        const size_t want = (size_t)(L * P * T * (det ? D : 0) + L * P * T * (pol ? nb : 0) + L * P * M + ((what & msl::LR_PACBED) ? L * M : 0));
        good = y.total == want && y.diff_off == 0 && (y.diff_layer % 2 == 0 || M % 2 != 0);
        std::unique_ptr<uint8_t[]> hits(new uint8_t[y.total ? y.total : 1]());
        double* base = nullptr;                                   // offsets only: nothing is dereferenced through it
        (void)base;
        for (int64_t l = 0; l < L; ++l) {
            for (int64_t r = 0; det && r < P * T; ++r)            // rows b * count + j of the largest sequence, count = T
                for (int64_t d = 0; d < D; ++d) ++hits[y.det(l) + (size_t)(r * D + d)];
            for (int64_t r = 0; pol && r < P * T; ++r)
                for (int64_t b = 0; b < nb; ++b) ++hits[y.pol(l) + (size_t)(r * nb + b)];
            for (int64_t p = 0; pat && p < P; ++p)
                for (int64_t m = 0; m < M; ++m) ++hits[y.diff(l) + (size_t)(p * M + m)];
            for (int64_t m = 0; (what & msl::LR_PACBED) && m < M; ++m) ++hits[y.acc(l) + (size_t)m];
        }
        for (size_t i = 0; i < y.total; ++i) good = good && hits[i] == 1;
    }
    std::printf("what=%-2u L=%-3lld P=%-3lld T=%-2lld D=%-2lld bins=%-4lld %lldx%-3lld %s\n", what, (long long)L, (long long)P, (long long)T, (long long)D,
                (long long)nb, (long long)mx, (long long)my, good ? "ok" : "FAILED");
    failures += !good;
}

static void refuse(const char* name, bool ok) {
    std::printf("%-40s %s\n", name, !ok ? "ok" : "FAILED");
    failures += ok;
}

int main() {
    for (unsigned what = 1; what <= msl::LR_ALL; ++what)
        for (int64_t L : {1, 3, 6}) check(what, L, 2, 2, 3, 12, 16, 16);
    check(msl::LR_ALL, 21, 5, 3, 16, 7, 3, 5);                  // odd pattern sizes: no 16-byte promise, every offset still exact
    check(msl::LR_DETECT | msl::LR_PACBED, 2, 1, 1, 1, 0, 1, 1);
    check(msl::LR_POLAR, 4, 7, 1, 0, 4096, 0, 0);
    msl::LrLayout y;
    refuse("no reduction", msl::lr_layout(0, 2, 2, 2, 3, 12, 16, 16, &y));
    refuse("an unknown bit", msl::lr_layout(16, 2, 2, 2, 3, 12, 16, 16, &y));
    refuse("no layer", msl::lr_layout(1, 0, 2, 2, 3, 12, 16, 16, &y));
    refuse("detect without detectors", msl::lr_layout(1, 2, 2, 2, 0, 12, 16, 16, &y));
    refuse("polar without bins", msl::lr_layout(2, 2, 2, 2, 3, 0, 16, 16, &y));
    refuse("patterns of no pixel", msl::lr_layout(4, 2, 2, 2, 3, 12, 0, 16, &y));
    refuse("overflow", msl::lr_layout(4, (int64_t)1 << 30, (int64_t)1 << 30, 2, 3, 12, 1 << 20, 1 << 20, &y));
    std::printf(failures ? "%d FAILED\n" : "all ok\n", failures);
    return failures != 0;
}
