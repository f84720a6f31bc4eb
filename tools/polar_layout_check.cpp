// Stand-alone check of the polar detector's pixel layout (pyslice_amd/csrc/polar.h: polar_layout), for a host sanitizer:
//   c++ -std=c++17 -g -O1 -fsanitize=address,undefined -o polar_layout_check tools/polar_layout_check.cpp && ./polar_layout_check
// Every buffer has exactly the size the ABI asks for (K bins, K order entries, n_bins + 1 segment bounds), so a write or read one
// element out of bounds is an error under the sanitizer; the result is compared with std::stable_sort.  Needs no device.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <memory>
#include <numeric>
#include <random>

#include "../pyslice_amd/csrc/polar.h"

static int failures = 0;

static void check(const char* name, const uint16_t* bin, int64_t K, int32_t n_bins, bool want_ok) {
    std::unique_ptr<uint32_t[]> order(new uint32_t[K > 0 ? K : 1]);
    std::unique_ptr<int64_t[]> seg(new int64_t[n_bins + 1]);
    const bool ok = msl::polar_layout(bin, K, n_bins, order.get(), seg.get());
    bool good = ok == want_ok;
    if (ok && want_ok) {
        std::vector<uint32_t> ref;
        for (int64_t k = 0; k < K; ++k)
            if (bin[k] != msl::POLAR_NONE) ref.push_back((uint32_t)k);
        std::stable_sort(ref.begin(), ref.end(), [&](uint32_t a, uint32_t b) { return bin[a] < bin[b]; });
        good = seg[0] == 0 && seg[n_bins] == (int64_t)ref.size() && std::equal(ref.begin(), ref.end(), order.get());
        for (int32_t b = 0; good && b < n_bins; ++b)
            for (int64_t i = seg[b]; i < seg[b + 1]; ++i) good = good && bin[order[i]] == b;
    }
    std::printf("%-16s K=%-6lld n_bins=%-5d %s\n", name, (long long)K, n_bins, good ? "ok" : "FAILED");
    failures += !good;
}

int main() {
    std::mt19937 rng(7);
    for (int32_t n_bins : {1, 7, 4096}) {
        const int64_t K = 5000;
        std::unique_ptr<uint16_t[]> m(new uint16_t[K]);
        for (int64_t k = 0; k < K; ++k) m[k] = rng() % 10 < 3 ? msl::POLAR_NONE : (uint16_t)(rng() % n_bins);
        check("random", m.get(), K, n_bins, true);
    }
    {
        std::unique_ptr<uint16_t[]> m(new uint16_t[300]);
        std::fill(m.get(), m.get() + 300, msl::POLAR_NONE);
        check("all none", m.get(), 300, 5, true);
    }
    {
        const uint16_t ids[3] = {2, 5, 11};
        std::unique_ptr<uint16_t[]> m(new uint16_t[777]);
        for (int k = 0; k < 777; ++k) m[k] = ids[rng() % 3];
        check("empty bins", m.get(), 777, 13, true);
        check("last bin only", m.get(), 777, 12, true);
        check("id == n_bins", m.get(), 777, 11, false);
    }
    {
        std::unique_ptr<uint16_t[]> m(new uint16_t[1]);
        m[0] = 3;
        check("K = 1", m.get(), 1, 4, true);
        check("K = 1, id 3 of 3", m.get(), 1, 3, false);
        m[0] = msl::POLAR_NONE;
        check("K = 1, none", m.get(), 1, 4, true);
        check("K = 0", m.get(), 0, 4, true);
    }
    {
        const int64_t K = 256 * 256;                   // every bin id once and more, the largest map id next to MSL_POLAR_NONE
        std::unique_ptr<uint16_t[]> m(new uint16_t[K]);
        for (int64_t k = 0; k < K; ++k) m[k] = (uint16_t)(k % 4097 == 4096 ? msl::POLAR_NONE : k % 4097);
        check("4096 bins full", m.get(), K, 4096, true);
    }
    std::printf(failures ? "%d FAILED\n" : "all ok\n", failures);
    return failures ? 1 : 0;
}
