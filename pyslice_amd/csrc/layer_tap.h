// Thickness series (msl_set_layers): the layer tap and the layered complex128 download.
//
//   layer_tap_gather_kernel   S = A_d psi_k, as the pass of slice k left it in its work buffer -- layout A ([x][y]) or B ([y][x]),
//                             lines in natural, interleaved or paired-lines order -- into a natural [x][y]
//                             image set, optionally times a weight per y (the two-pass loop: conj(P_y), undoing the propagator
//                             half the row pass applied).  The FFTs and the exit epilogue then run on that copy.
//   layer_tap_c128_kernel     (L, P, T, pitch) c64 -> (P, T, wx*wy, L) c128 chunk: the reference's layer axis last.
#pragma once

#include <hip/hip_runtime.h>

namespace msl {

enum { TAP_NATURAL = 0, TAP_INTERLEAVED = 1, TAP_PAIRED = 2 };

struct TapGatherJob {
    const float2* src;      // work buffer of the pass: (images, n_lines, src_pitch)
    float2* dst;            // (images, nx, dst_pitch), natural order
    const float2* wy;       // (ny) weight along y or null
    float wscale;           // factor of the weight
    long long src_is, dst_is;
    int src_pitch, dst_pitch;
    int nx, ny;
    int transposed;         // 1: source lines run along x, one per y (layout B)
    int order;              // TAP_NATURAL / TAP_INTERLEAVED (rp = R' of the reading kernel) / TAP_PAIRED (2048-point lines)
    int rp;
};

// element e of line L of the source image: offset in float2 units
__device__ __forceinline__ long long tap_src_offset(const TapGatherJob& j, int L, int e) {
    if (j.order == TAP_INTERLEAVED) {
        // position 2 R' (jj >> 1) + 2 l + (jj & 1) holds element R' jj + l (rowt_pass.h)
        const int jj = e / j.rp, l = e - jj * j.rp;
        return (long long)L * j.src_pitch + 2 * j.rp * (jj >> 1) + 2 * l + (jj & 1);
    }
    if (j.order == TAP_PAIRED) {
        // entry 256 (e >> 7) + (2 (e & 63) + (L & 1)) * 2 + ((e >> 6) & 1) of the row of pair L / 2 (fft_pow2.h: rowTW_pass_kernel)
        return (long long)(L >> 1) * (2 * j.src_pitch) + 256 * (e >> 7) + (2 * (e & 63) + (L & 1)) * 2 + ((e >> 6) & 1);
    }
    return (long long)L * j.src_pitch + e;
}

// Tile of TL source lines x TE elements through the LDS: the loads run along the source lines (the permutations of the interleaved
// and paired orders stay inside aligned blocks of 32 / 64 / 128 elements, so a wave's loads cover whole segments), the stores run
// along y of the natural image -- for a layout-B source that is across the source lines (transposition).
template <int TL, int TE>
__global__ void __launch_bounds__(256) layer_tap_gather_kernel(TapGatherJob j) {
    __shared__ float2 tile[TL][TE + 1];
    const int n_lines = j.transposed ? j.ny : j.nx;
    const int len = j.transposed ? j.nx : j.ny;
    const int e0 = blockIdx.x * TE, L0 = blockIdx.y * TL;
    const long long img = blockIdx.z;
    const float2* src = j.src + img * j.src_is;
    for (int i = threadIdx.x; i < TL * TE; i += 256) {
        const int li = i / TE, ei = i - li * TE;
        const int L = L0 + li, e = e0 + ei;
        if (L < n_lines && e < len) tile[li][ei] = src[tap_src_offset(j, L, e)];
    }
    __syncthreads();
    float2* dst = j.dst + img * j.dst_is;
    if (!j.transposed) {                   // line = x, element = y
        for (int i = threadIdx.x; i < TL * TE; i += 256) {
            const int li = i / TE, ei = i - li * TE;
            const int x = L0 + li, y = e0 + ei;
            if (x >= j.nx || y >= j.ny) continue;
            float2 v = tile[li][ei];
            if (j.wy) { const float2 w = j.wy[y]; v = make_float2((v.x * w.x - v.y * w.y) * j.wscale, (v.x * w.y + v.y * w.x) * j.wscale); }
            dst[(long long)x * j.dst_pitch + y] = v;
        }
    } else {                               // line = y, element = x
        for (int i = threadIdx.x; i < TL * TE; i += 256) {
            const int ei = i / TL, li = i - ei * TL;
            const int x = e0 + ei, y = L0 + li;
            if (x >= j.nx || y >= j.ny) continue;
            float2 v = tile[li][ei];
            if (j.wy) { const float2 w = j.wy[y]; v = make_float2((v.x * w.x - v.y * w.y) * j.wscale, (v.x * w.y + v.y * w.x) * j.wscale); }
            dst[(long long)x * j.dst_pitch + y] = v;
        }
    }
}

// out[i] for i < n * L: dense offset o = o0 + i / L of probe p's (T_used, wpix) frames, layer l = i % L
__global__ void __launch_bounds__(256) layer_tap_c128_kernel(const float2* __restrict__ layers, double2* __restrict__ out, long long o0,
                                                               long long n, int L, long long block, long long probe_off, long long wpix,
                                                               long long wpitch) {
    const long long total = n * L;
    for (long long i = blockIdx.x * 256LL + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const long long o = o0 + i / L;
        const int l = (int)(i % L);
        const long long t = o / wpix, px = o - t * wpix;
        const float2 v = layers[l * block + probe_off + t * wpitch + px];
        out[i] = make_double2((double)v.x, (double)v.y);
    }
}

}  // namespace msl
