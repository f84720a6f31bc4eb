// time_welch_kernel<L>: windowed, segment-averaged spectra, one lane per pixel (tacaw_welch.h) -- the 40 instantiations.
#include <algorithm>
#include "tacaw_welch.h"

namespace msl {

// segment lengths with a kernel: those of time_direct_kernel, the 2-3-5-7-smooth numbers in [TDIR_MIN, TDIR_MAX]
#define MSL_TWELCH_LENGTHS(X) X(16) X(18) X(20) X(24) X(25) X(27) X(30) X(32) X(36) X(40) X(45) X(48) X(50) X(54) X(60) X(64) X(72) X(75) \
    X(80) X(81) X(90) X(96) X(100) X(108) X(120) X(125) X(128) \
    X(21) X(28) X(35) X(42) X(49) X(56) X(63) X(70) X(84) X(98) X(105) X(112) X(126)

bool time_welch_has(int L) { return L >= TDIR_MIN && L <= TDIR_MAX && fft_smooth7(L); }

template <int L>
static bool launch_l(const WelchJob& j, int n_cus, hipStream_t stream) {
    static_assert(fft_smooth7(L) && L >= TDIR_MIN && L <= TDIR_MAX, "no per-lane Welch kernel for this segment length");
    const long long tiles = ((long long)(j.npix + 255) / 256) * j.n_images;
    int per_cu = 1;                                  // 1 for the long segments (512 registers per lane), more for the short ones
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, (const void*)time_welch_kernel<L>, 256, 0) != hipSuccess || per_cu < 1) per_cu = 1;
    const int grid = (int)std::min<long long>(tiles, (long long)n_cus * per_cu);
    hipLaunchKernelGGL((time_welch_kernel<L>), dim3(grid), dim3(256), 0, stream, j);
    return true;
}

bool time_welch_launch(const WelchJob& j, int n_cus, hipStream_t stream) {
    switch (j.L) {
#define X(n) case n: return launch_l<n>(j, n_cus, stream);
        MSL_TWELCH_LENGTHS(X)
#undef X
    }
    return false;
}

}  // namespace msl
