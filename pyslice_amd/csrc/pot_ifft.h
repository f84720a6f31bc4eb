// Inverse FFT passes of the potential build: V_s = Re ifft2(R_s) / (dx^2 dy^2), t_s = exp(i sigma V_s) (potentials.py:336-342,
// multislice.py:282).  Every form is two passes of one kernel family: a pass inverse-transforms the lines of a stack and stores them
// TRANSPOSED through a tile in the LDS, so two passes give ifft2 with the data back in its natural layout; the second pass reads a
// half spectrum (job.herm), applies the potential epilogue and writes a slice either transposed back or as rows (the orientation
// the passes along x read).
//
//   ifftT2_kernel      512-point lines (2 R^2, line2_transform); PAIR: two real lines per complex transform
//   ifftTB_kernel      any length <= R^2 / 2 by chirp-z on the four-step register FFT; PAIR likewise
//   ifftTB_two_kernel  the same transform, first pass only: two lines per group and tile round
//   ifftTB2_kernel     513..1024 points by chirp-z on the wave-per-line 2048-point FFT
//   ifftTW_kernel      2048-point lines, one wave per line
//
// The steps the kernels share are written once, ahead of them; each kernel body reads load -> (combine) -> transform -> epilogue ->
// store.  Next to each kernel stands the description of its LDS (Ifft*Lds): the kernel takes its offsets from it, its launcher
// (mslice.hip) the bytes and the lines per work item.
#pragma once
#include "fft_pow2.h"

namespace msl {

struct IfftJob {
    const float2* in;           // (n_images, n_lines, in_pitch): lines of n_line points in natural frequency order
    float2* out_t;              // transposed store: out_t[img][pos][line]
    float2* out_rows;           // row store (potential epilogue only): out_rows[img][line][pos]
    const float2* tw;           // four-step twiddles of length R^2 (ifftTB2 / ifftTW_kernel: the 2048-point wave FFT's T table)
    const float2* tw2;          // ifftT2_kernel: W_512^m; ifftTB2 / ifftTW_kernel: W_64 table
    const float2* bf;           // chirp filter, first half + 1
    const float2* bw;           // chirp, zero beyond n_line
    long long in_is, out_t_is, out_rows_is;
    int in_pitch, out_t_pitch, out_rows_pitch, n_lines, n_line, n_images;      // (ifftT2 / ifftTW_kernel: n_line is their fixed length)
    int potential;              // 1: V = Re(.) * scale, out = exp(i sigma V)
    int rows_parity;            // potential: images whose slice number has this parity are stored as rows, the others transposed; -1: none
    int slice_mod;              // slice number of image img = img % slice_mod (several frames' stacks in one launch); 0: img itself
    int herm;                   // 1: only elements 0 .. n_line/2 of an input line exist, the others are conj(line[n_line - e]) (spectrum of a real image)
    float scale, sigma_over_pi;
};

constexpr size_t IFFT_LDS_MAX = 160 * 1024;      // msl_handle::lds_limit's default: every layout below fits it

// ---- the shared steps -------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ const float2* in_line(const IfftJob& job, int img, int line) {
    return job.in + (long long)img * job.in_is + (long long)line * job.in_pitch;
}
__device__ __forceinline__ float2* out_row(const IfftJob& job, int img, int line) {
    return job.out_rows + (long long)img * job.out_rows_is + (long long)line * job.out_rows_pitch;
}
__device__ __forceinline__ float2* out_col(const IfftJob& job, int img, int col) { return job.out_t + (long long)img * job.out_t_is + col; }

// slice number of an image of a potential-build launch (the stacks of several frames follow each other)
__device__ __forceinline__ int slice_of(const IfftJob& job, int img) { return job.slice_mod > 0 ? img % job.slice_mod : img; }
// workgroup-uniform: this slice is kept as rows
__device__ __forceinline__ bool stored_as_rows(const IfftJob& job, int img) { return job.potential && (slice_of(job, img) & 1) == job.rows_parity; }

// Element e of a line of n points of which 0 .. hx exist: the others are conj(line[n - e]), left unconjugated with RAW.  hx = n / 2
// for the spectrum of a real line (job.herm), n for a whole line.  GUARD: zero from n on.
__device__ __forceinline__ int mirror_point(const IfftJob& job, int n) { return job.herm ? n / 2 : n; }
template <bool GUARD, bool RAW = false>
__device__ __forceinline__ float2 herm_load(const float2* src, int e, int n, int hx) {
    float2 x = (!GUARD || e < n) ? src[e <= hx ? e : n - e] : make_float2(0.f, 0.f);
    if (!RAW && e > hx) x.y = -x.y;
    return x;
}
// dst[j] <- element j STRIDE + ln, j < COUNT
template <int STRIDE, int COUNT, bool GUARD, int RN>
__device__ __forceinline__ void load_elements(float2 (&dst)[RN], const float2* src, int ln, int n, int hx) {
#pragma unroll
    for (int j = 0; j < COUNT; ++j) dst[j] = herm_load<GUARD>(src, j * STRIDE + ln, n, hx);
}

// Two real lines on one complex transform, Z = X_a + i X_b -> V_a + i V_b: element e of Z from the RAW elements of the two half
// spectra, a + i b below the mirror point, conj(a) + i conj(b) above it.  The Nyquist element of an even length is its own mirror
// image: only its real part belongs to a real line (an unpaired transform drops the rest with the imaginary part of its output;
// here it would land in the partner line).
__device__ __forceinline__ float2 pair_combine(float2 a, float2 b, int e, int n) {
    if (2 * e == n) a.y = b.y = 0.f;
    return (e <= n / 2) ? make_float2(a.x - b.y, a.y + b.x) : make_float2(a.x + b.y, b.x - a.y);
}

// x conj(w): the chirp table is zero beyond the line, the upper half of the registers is padding
template <int STRIDE, int TCH, int R>
__device__ __forceinline__ void mul_chirp(float2 (&v)[R], const float2* bw, int ln) {
#pragma unroll
    for (int c = 0; c < R / 2; c += TCH) {
        float2 w[TCH];
#pragma unroll
        for (int j = 0; j < TCH; ++j) w[j] = bw[(c + j) * STRIDE + ln];
#pragma unroll
        for (int j = 0; j < TCH; ++j) v[c + j] = cmulf_conj(v[c + j], w[j]);
        __builtin_amdgcn_sched_barrier(0);
    }
#pragma unroll
    for (int j = R / 2; j < R; ++j) v[j] = make_float2(0.f, 0.f);
}
// x conj(Bf): fa = bf + lane, fb = bf - lane, the filter's first half + 1 read from both ends
template <int STRIDE, int TCH, int R>
__device__ __forceinline__ void mul_filter(float2 (&v)[R], const float2* fa, const float2* fb) {
#pragma unroll
    for (int c = 0; c < R; c += TCH) {
        float2 w[TCH];
#pragma unroll
        for (int j = 0; j < TCH; ++j) w[j] = (c + j < R / 2) ? fa[(c + j) * STRIDE] : fb[(R - (c + j)) * STRIDE];
#pragma unroll
        for (int j = 0; j < TCH; ++j) v[c + j] = cmulf_conj(v[c + j], w[j]);
        __builtin_amdgcn_sched_barrier(0);
    }
}
// inverse n-point DFT of a line in the lower half of v by chirp-z on the four-step register FFT of length R^2 >= 2 n,
// x = conj(w) . IFFT(FFT(pad(X conj(w))) conj(Bf)) (the inverse of rowTB_pass_kernel's chirp-z form: same tables)
template <int R, int TCH>
__device__ __forceinline__ void chirpz_inverse(float2 (&v)[R], const float* wscr, unsigned wscr_lds, const float2* tw, const float2* bw,
                                               const float2* fa, const float2* fb, int ln, int lane64) {
    mul_chirp<R, TCH>(v, bw, ln);
    fourstep_split_addtid<R, false, TCH>(v, wscr, wscr_lds, tw, ln, lane64);
    mul_filter<R, TCH>(v, fa, fb);
    fourstep_split_addtid<R, true, TCH>(v, wscr, wscr_lds, tw, ln, lane64);
    mul_chirp<R, TCH>(v, bw, ln);
}

// exp(i sigma V) through sincospi: its range reduction is exact, where sincosf carries a slow path with a private array (scratch);
// sigma / pi is formed in double on the host.
__device__ __forceinline__ float2 transmission_of(const IfftJob& job, float x) {
    float sn, cs;
    sincospif(job.sigma_over_pi * (x * job.scale), &sn, &cs);
    return make_float2(cs, sn);
}
// v[j] <- exp(i sigma V) of x(j), j < COUNT: four rounds in flight, not all of them
template <int COUNT, int RN, typename X>
__device__ __forceinline__ void apply_transmission(const IfftJob& job, float2 (&v)[RN], X x) {
#pragma unroll
    for (int j = 0; j < COUNT; ++j) {
        if (j % 4 == 0) __builtin_amdgcn_sched_barrier(0);
        v[j] = transmission_of(job, x(j));
    }
}
template <int COUNT, int RN>
__device__ __forceinline__ void apply_transmission(const IfftJob& job, float2 (&v)[RN]) {
    apply_transmission<COUNT>(job, v, [&](int j) { return v[j].x; });
}

// dst[j STRIDE + ln] <- v[J0 + j], j < COUNT: a line into its row of the tile, or (GUARD: the elements below n) of the row store
template <int STRIDE, int COUNT, int J0 = 0, bool GUARD = false, int RN>
__device__ __forceinline__ void put_line(float2* dst, const float2 (&v)[RN], int ln, int n = 0) {
#pragma unroll
    for (int j = 0; j < COUNT; ++j) if (!GUARD || j * STRIDE + ln < n) dst[j * STRIDE + ln] = v[J0 + j];
}

// Transposed store of a tile of LINES rows (pitch PITCH) of NPOS positions, one thread per (position, line): a tile row lands as one
// run of 8 LINES bytes.  GUARD: the buffers are dense (pitch = line count, any parity), lines from job.n_lines and positions from n
// on are left out.  The 32-line tile keeps line g + 16 h in row 2 g + h (a wave's four rows are contiguous and hold its exchange
// scratch without reaching into another wave's rows).
template <int LINES, int NT, int NPOS, int PITCH, bool GUARD = true>
__device__ __forceinline__ void store_tile_transposed(const IfftJob& job, const float2* tile, int img, int col0, int tid, int n = NPOS) {
    constexpr int POS_PER_IT = NT / LINES;
    const int li = tid % LINES;
    int r0 = tid / LINES;
    if constexpr (LINES == 32) asm volatile("" : "+v"(r0));     // (laundered: 32 row offsets of 64 bits would be kept across the item loop)
    if (!GUARD || col0 + li < job.n_lines) {
        float2* dst = out_col(job, img, col0 + li);
        const float2* srow = tile + (LINES == 32 ? 2 * (li & 15) + (li >> 4) : li) * PITCH;
#pragma unroll
        for (int i = 0; i < NPOS / POS_PER_IT; ++i) {
            const int pos = r0 + POS_PER_IT * i;
            if (!GUARD || pos < n) dst[(long long)pos * job.out_t_pitch] = srow[pos];
        }
    }
}

template <int NT>
__device__ __forceinline__ void stage_table(float2* dst, const float2* src, int count, int tid) {
    for (int i = tid; i < count; i += NT) dst[i] = src[i];
}
// tables of the 2048-point wave FFT: T in lane order (lds_pos64), W_64
template <int NT>
__device__ __forceinline__ void stage_wave2k_tables(float2* tw, float2* w64, const IfftJob& job, int tid) {
    for (int i = tid; i < 2048; i += NT) tw[lds_pos64(i)] = job.tw[i];
    if (tid < 64) w64[tid] = job.tw2[tid];
}

// ---- lines of 2 R^2 = 512 points: the potential build on 512 x 512 grids --------------------------------------------------------
// The inverse transform went through the generic LDS kernel on these grids (two passes at 2.6 TB/s plus a transposition of every
// second slice; 0.35 of 0.73 ms per frame at 512^2 x 100, which a single probe cannot amortise).  Two passes of this kernel
// instead: the line is loaded in the split order the register transform wants -- slot k of set b is X[2k + b], i.e. one 16-byte
// load per lane and register -- inverse-transformed (line2_transform) and stored transposed through the 16-line tile.
template <int R, bool PAIR = false>
struct IfftT2Lds {
    static constexpr int N2 = R * R, N = 2 * N2, NT = 16 * R;
    static constexpr int LINES = PAIR ? 32 : 16;                  // lines per work item
    static constexpr int LINE_BLOCK = LINES;                      // no guards: the line count is a multiple of it
    static constexpr int CS = N + 1;                              // tile row pitch
    static constexpr int TW = 0, TW2 = TW + N2, TILE = TW2 + N2;  // (float2) the tile: 16 rows, also the transpose scratch
    static constexpr size_t bytes = (size_t)(TILE + 16 * CS) * sizeof(float2);
    static_assert(bytes <= IFFT_LDS_MAX, "ifftT2_kernel: LDS");
};

// PAIR (second pass: job.herm and job.potential set, line count a multiple of 32): a group takes the lines g and g + 16 of a
// 32-line block (pair_combine).  Line a of the next item is prefetched in registers as before, line b arrives at the top of the
// item (two prefetched lines do not fit).
template <int R, bool PAIR = false>
__global__ void __launch_bounds__(16 * R, 2) ifftT2_kernel(IfftJob job) {
    static_assert(R == 16, "512-point lines only (64 complex values per lane at R = 32 spill: 2048-point axes use ifftTW_kernel)");
    using Lds = IfftT2Lds<R, PAIR>;
    constexpr int N2 = Lds::N2, N = Lds::N, NT = Lds::NT, BL = Lds::LINES, CS = Lds::CS;
    constexpr int POS_PER_IT = NT / 8;
    constexpr int NIT = N / POS_PER_IT;
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    float2* tw = reinterpret_cast<float2*>(smem_raw) + Lds::TW;
    float2* tw2 = reinterpret_cast<float2*>(smem_raw) + Lds::TW2;
    float2* tile = reinterpret_cast<float2*>(smem_raw) + Lds::TILE;
    const int tid = threadIdx.x;
    stage_table<NT>(tw, job.tw, N2, tid);
    stage_table<NT>(tw2, job.tw2, N2, tid);
    __syncthreads();
    const int grp = tid / R, ln = tid % R;
    const int q = tid & 7, r0 = tid >> 3;
    float* scratch = reinterpret_cast<float*>(tile + grp * CS);
    const int lblocks = job.n_lines / BL;
    const int n_items = lblocks * job.n_images;
    // the next item's line is loaded into registers while the current one is transformed (two 256-thread workgroups per CU = two
    // waves per SIMD: without it the loads of an item were exposed -- 193 us of a 0.33 ms potential per frame at 512^2 x 100)
    float2 vn[2 * R];
    // slot j of set b <- element 2 (j R + ln) + b of line `line`; with herm the mirrored element (conjugated unless PAIR: raw)
    auto load_line = [&](int it, int line_in_block, float2 (&dst)[2 * R]) {
        const int img = it / lblocks, lb = it - img * lblocks;
        const float2* src = in_line(job, img, lb * BL + line_in_block);
        int lnl = ln;
        asm volatile("" : "+v"(lnl));
        if (job.herm) {                                     // workgroup-uniform: mirrored elements as two 8-byte loads
#pragma unroll
            for (int j = 0; j < R; ++j) {
                // (herm_load's rule spelled out on the two elements of a slot pair: through the shared function this kernel takes
                // 44 more SGPRs and, with PAIR, 256 VGPRs and 188 bytes of scratch)
                const int e0 = 2 * (j * R + lnl), e1 = e0 + 1;
                float2 a = src[e0 <= N / 2 ? e0 : N - e0], b = src[e1 <= N / 2 ? e1 : N - e1];
                if (!PAIR && e0 > N / 2) a.y = -a.y;
                if (!PAIR && e1 > N / 2) b.y = -b.y;
                dst[j] = a; dst[R + j] = b;
            }
        } else {
#pragma unroll
            for (int j = 0; j < R; ++j) {
                const float4 x = *reinterpret_cast<const float4*>(src + 2 * (j * R + lnl));
                dst[j] = make_float2(x.x, x.y); dst[R + j] = make_float2(x.z, x.w);
            }
        }
    };
    if ((int)blockIdx.x < n_items) load_line(blockIdx.x, grp, vn);
    for (int item = blockIdx.x; item < n_items; item += gridDim.x) {
        const int img = item / lblocks, lb = item - img * lblocks;
        int lnv = ln;                                       // laundered: keeps dozens of per-lane LDS / global addresses from being
        asm volatile("" : "+v"(lnv));                       // hoisted out of the loop into registers the transform needs
        float2 v[2 * R];
        if constexpr (PAIR) {
            float2 vb[2 * R];
            load_line(item, 16 + grp, vb);
#pragma unroll
            for (int j = 0; j < 2 * R; ++j) v[j] = pair_combine(vn[j], vb[j], 2 * ((j % R) * R + lnv) + j / R, N);
        } else {
#pragma unroll
            for (int j = 0; j < 2 * R; ++j) v[j] = vn[j];
        }
        __builtin_amdgcn_sched_barrier(0);
        if (item + (int)gridDim.x < n_items) load_line(item + (int)gridDim.x, grp, vn);
        __builtin_amdgcn_sched_barrier(0);
        float* scr = scratch;
        asm volatile("" : "+v"(scr));
        line2_transform<R, true>(v, scr, tw, tw2, lnv);
        float vy[PAIR ? 2 * R : 1];
        if constexpr (PAIR) {
#pragma unroll
            for (int j = 0; j < 2 * R; ++j) vy[j] = v[j].y;
        }
        const bool as_rows = stored_as_rows(job, img);
#pragma unroll
        for (int half = 0; half < (PAIR ? 2 : 1); ++half) {
            if (job.potential) apply_transmission<2 * R>(job, v, [&](int j) { return half == 0 ? v[j].x : vy[j]; });
            if (as_rows) {                                  // (split order: slot j of set b is position b N2 + j R + lane)
                float2* dst = out_row(job, img, lb * BL + half * 16 + grp);
#pragma unroll
                for (int j = 0; j < 2 * R; ++j) dst[(j / R) * N2 + (j % R) * R + lnv] = v[j];
                continue;
            }
            // the 16-line tile leaves two lines per thread, in 16-byte streaming stores
            float2* dst = out_col(job, img, lb * BL + half * 16);
            int off0 = 2 * q + r0 * job.out_t_pitch;
            asm volatile("" : "+v"(off0));
            const int ostep = POS_PER_IT * job.out_t_pitch;
            lds_barrier();                             // the tile (and every group's scratch use) is free
            put_line<R, N / R>(reinterpret_cast<float2*>(scr), v, lnv);
            lds_barrier();
#pragma unroll
            for (int i = 0; i < NIT; ++i) {
                const int pos = r0 + POS_PER_IT * i;
                const float2 a = tile[(2 * q) * CS + pos], b = tile[(2 * q + 1) * CS + pos];
                st_stream(dst + (off0 + i * ostep), a.x, a.y, b.x, b.y);
            }
        }
        if (!as_rows) lds_barrier();
    }
}

// ---- any length up to R^2 / 2 (grid lengths that are not powers of two) by chirp-z on the four-step register FFT --------------------
// Replaces the generic LDS-resident Bluestein kernel in that role (501^2 x 100 slices: 2 x 500 us -> 2 x ~90 us per frame: for the
// reference's default single-probe runs the inverse transform of the potential WAS the frame).  The buffers are dense (pitch =
// line count, any parity): stores are 8 bytes per line and guarded, a tile row still lands as one 128-byte run.

// the LDS of a chirp-z kernel: the FFT's tables (TABLES float2), the chirp filter bf (NH + 2), the chirp bw (NH), then the tile
template <int TABLES, int NH>
struct IfftCzLds {
    static constexpr int TW = 0, BF = TABLES, BW = BF + NH + 2, TILE = BW + NH;
    static constexpr int LINE_BLOCK = 1;                          // guarded loads and stores: any line count
};
template <int R, bool PAIR = false>
struct IfftTBLds : IfftCzLds<R * R, R * R / 2> {
    static constexpr int M = R * R, NH = M / 2, GROUPS = 16, NT = GROUPS * R;
    static constexpr int LINES = PAIR ? 2 * GROUPS : GROUPS;      // lines per work item
    static constexpr int CS = R * (R + 1) + 2;                    // row pitch of the 16-line tile
    // PAIR: a 32-row tile of the NH positions (pitch CSP) -- both lines of a group leave in ONE round of 256-byte runs, and a
    // wave's four contiguous rows hold its exchange scratch (ifftTB_two_kernel's layout)
    static constexpr int CSP = NH + 2;
    static constexpr size_t bytes = (size_t)(IfftTBLds::TILE + GROUPS * CS) * sizeof(float2);
    static_assert(!PAIR || (R == 32 && 4 * CSP >= R * 68 / 2 && 2 * GROUPS * CSP <= GROUPS * CS), "paired lines: 1024-point transforms only");
    static_assert(bytes <= IFFT_LDS_MAX, "ifftTB_kernel: LDS");
};

// PAIR (second pass of the potential build: job.herm and job.potential set): the lines are spectra of REAL lines, so two of them
// ride one complex transform (pair_combine) -- half the transforms of this pass.  A group takes the lines g and g + 16 of a
// 32-line block; both leave through one 32-row tile round (256-byte runs).
template <int R, bool PAIR = false>
__global__ void __launch_bounds__(16 * R, (R == 32) ? 2 : 4) ifftTB_kernel(IfftJob job) {
    using Lds = IfftTBLds<R, PAIR>;
    constexpr int H = R / 2, NH = Lds::NH, GROUPS = Lds::GROUPS, NT = Lds::NT, BL = Lds::LINES, CS = Lds::CS, CSP = Lds::CSP, TCH = 8;
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    float2* tw = reinterpret_cast<float2*>(smem_raw) + Lds::TW;
    float2* bf = reinterpret_cast<float2*>(smem_raw) + Lds::BF;
    float2* bw = reinterpret_cast<float2*>(smem_raw) + Lds::BW;
    float2* tile = reinterpret_cast<float2*>(smem_raw) + Lds::TILE;
    const int tid = threadIdx.x;
    const int N = job.n_line;
    stage_table<NT>(tw, job.tw, Lds::M, tid);
    stage_table<NT>(bf, job.bf, NH + 1, tid);
    stage_table<NT>(bw, job.bw, NH, tid);
    __syncthreads();
    const int grp = tid / R, ln = tid % R;
    float2* myrow = PAIR ? tile + (2 * grp) * CSP : tile + grp * CS;
    float2* const wtile = PAIR ? tile + (4 * (grp / 2)) * CSP : tile + (grp - grp % (64 / R)) * CS;
    const float* wscr = reinterpret_cast<const float*>(wtile);
    const unsigned wscr_lds = __builtin_amdgcn_readfirstlane((unsigned)(size_t)wtile);
    const float2* fa = bf + ln;
    const float2* fb = bf - ln;
    const int lblocks = (job.n_lines + BL - 1) / BL;
    const int n_items = lblocks * job.n_images;
    // the next item's line is loaded into registers while the current one is transformed
    float2 vn[PAIR ? R : H];
    auto load_line = [&](int it) {
        const int img = it / lblocks, lb = it - img * lblocks;
        const float2* src = in_line(job, img, min(lb * BL + grp, job.n_lines - 1));     // surplus lines of the last block repeat the last one
        const int hx = mirror_point(job, N);
        if constexpr (PAIR) {
            const float2* srcb = in_line(job, img, min(lb * BL + GROUPS + grp, job.n_lines - 1));
#pragma unroll
            for (int j = 0; j < H; ++j) {
                vn[j] = herm_load<true, true>(src, j * R + ln, N, hx);
                vn[H + j] = herm_load<true, true>(srcb, j * R + ln, N, hx);
            }
        } else {
            load_elements<R, H, true>(vn, src, ln, N, hx);
        }
    };
    if ((int)blockIdx.x < n_items) load_line(blockIdx.x);
    for (int item = blockIdx.x; item < n_items; item += gridDim.x) {
        const int img = item / lblocks, lb = item - img * lblocks;
        const int L = min(lb * BL + grp, job.n_lines - 1);
        float2 v[R];
        if constexpr (PAIR) {
#pragma unroll
            for (int j = 0; j < H; ++j) v[j] = pair_combine(vn[j], vn[H + j], j * R + ln, N);
        } else {
#pragma unroll
            for (int j = 0; j < H; ++j) v[j] = vn[j];
        }
        __builtin_amdgcn_sched_barrier(0);
        if (item + (int)gridDim.x < n_items) load_line(item + (int)gridDim.x);
        __builtin_amdgcn_sched_barrier(0);
        chirpz_inverse<R, TCH>(v, wscr, wscr_lds, tw, bw, fa, fb, ln, tid & 63);
        if constexpr (PAIR) {                                  // v[j] = V_a + i V_b: t_a into v[j], t_b into v[H + j]
#pragma unroll
            for (int j = 0; j < H; ++j) {
                if (j % 4 == 0) __builtin_amdgcn_sched_barrier(0);
                const float2 ta = transmission_of(job, v[j].x), tb = transmission_of(job, v[j].y);
                v[j] = ta;
                v[H + j] = tb;
            }
        } else if (job.potential) {
            apply_transmission<H>(job, v);
        }
        if (stored_as_rows(job, img)) {
            if (lb * BL + grp < job.n_lines) put_line<R, H, 0, true>(out_row(job, img, L), v, ln, N);
            if constexpr (PAIR) {
                if (lb * BL + GROUPS + grp < job.n_lines) put_line<R, H, H, true>(out_row(job, img, lb * BL + GROUPS + grp), v, ln, N);
            }
            continue;
        }
        wave_lds_fence();
        put_line<R, H>(myrow, v, ln);
        if constexpr (PAIR) put_line<R, H, H>(myrow + CSP, v, ln);
        lds_barrier();
        if constexpr (PAIR) store_tile_transposed<BL, NT, NH, CSP>(job, tile, img, lb * BL, tid, N);
        else store_tile_transposed<BL, NT, NH, CS>(job, tile, img, lb * BL, tid, N);
        lds_barrier();
    }
}

// First pass of the potential build (no epilogue) with TWO lines per group and item: ifftTB_kernel spends one tile round -- write,
// barrier, 16 x (LDS read + store), barrier -- per transform, twice the share it has in the slice-loop kernels with their four
// transforms per line, and its vector pipe idles half the time (50 % busy against rowTB_pass_kernel's 82 %, profiles/r03_*).  Here
// a group transforms line g, parks the 16 result registers, transforms line g + 16, and ONE round stores the 32-line tile: 256-byte
// runs, half the barriers per line.  Tile rows hold the N <= 512 positions only (pitch 514); row 2 g + h is line g + 16 h
// (store_tile_transposed).  Line a of the next item is prefetched before the first transform, line b once the results are in
// the tile (it is needed a whole transform later).
struct IfftTBTwoLds : IfftCzLds<1024, 512> {
    static constexpr int R = 32, M = R * R, NH = M / 2, GROUPS = 16, NT = GROUPS * R;
    static constexpr int LINES = 2 * GROUPS;                      // lines per work item
    static constexpr int CSN = NH + 2;                            // tile row pitch (float2): 2 mod 32, as the 16-line tiles' 1058
    static constexpr size_t bytes = (size_t)(TILE + LINES * CSN) * sizeof(float2);
    static_assert(4 * CSN >= R * 68 / 2, "a wave's four tile rows hold its exchange scratch (R rows x 68 floats)");
    static_assert(bytes <= IFFT_LDS_MAX, "ifftTB_two_kernel: LDS");
};

__global__ void __launch_bounds__(512, 2) ifftTB_two_kernel(IfftJob job) {
    using Lds = IfftTBTwoLds;
    constexpr int R = Lds::R, H = R / 2, NH = Lds::NH, GROUPS = Lds::GROUPS, BL = Lds::LINES, NT = Lds::NT, CSN = Lds::CSN, TCH = 8;
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    float2* tw = reinterpret_cast<float2*>(smem_raw) + Lds::TW;
    float2* bf = reinterpret_cast<float2*>(smem_raw) + Lds::BF;
    float2* bw = reinterpret_cast<float2*>(smem_raw) + Lds::BW;
    float2* tile = reinterpret_cast<float2*>(smem_raw) + Lds::TILE;
    const int tid = threadIdx.x;
    const int N = job.n_line;
    stage_table<NT>(tw, job.tw, Lds::M, tid);
    stage_table<NT>(bf, job.bf, NH + 1, tid);
    stage_table<NT>(bw, job.bw, NH, tid);
    __syncthreads();
    const int grp = tid / R, ln = tid % R;
    float2* rowa = tile + (2 * grp) * CSN;                    // my two rows: lines grp and grp + 16
    const float* wscr = reinterpret_cast<const float*>(tile + (4 * (grp / 2)) * CSN);
    const unsigned wscr_lds = __builtin_amdgcn_readfirstlane((unsigned)(size_t)(tile + (4 * (grp / 2)) * CSN));
    const float2* fa = bf + ln;
    const float2* fb = bf - ln;
    const int lblocks = (job.n_lines + BL - 1) / BL;
    const int n_items = lblocks * job.n_images;
    float2 vna[H], vnb[H];
    auto load_line = [&](int it, int h, float2 (&dst)[H]) {
        const int img = it / lblocks, lb = it - img * lblocks;
        const float2* src = in_line(job, img, min(lb * BL + h * GROUPS + grp, job.n_lines - 1));      // surplus lines of the last block repeat the last one
        int lnl = ln;                                       // laundered: the 16 element indices are the same for every item, and
        asm volatile("" : "+v"(lnl));                       // the compiler would keep them all in registers across the loop (and spill)
        load_elements<R, H, true>(dst, src, lnl, N, mirror_point(job, N));
    };
    if ((int)blockIdx.x < n_items) { load_line(blockIdx.x, 0, vna); load_line(blockIdx.x, 1, vnb); }
    for (int item = blockIdx.x; item < n_items; item += gridDim.x) {
        const int img = item / lblocks, lb = item - img * lblocks;
        // (the last item of a workgroup prefetches itself again: a conditional load would keep the old registers alive as the other
        // arm of the merge)
        const int nitem = item + (int)gridDim.x < n_items ? item + (int)gridDim.x : item;
        float2 v[R];
#pragma unroll
        for (int j = 0; j < H; ++j) v[j] = vna[j];
        __builtin_amdgcn_sched_barrier(0);
        load_line(nitem, 0, vna);
        __builtin_amdgcn_sched_barrier(0);
        chirpz_inverse<R, TCH>(v, wscr, wscr_lds, tw, bw, fa, fb, ln, tid & 63);
        float2 pa[H];
#pragma unroll
        for (int j = 0; j < H; ++j) { pa[j] = v[j]; v[j] = vnb[j]; }
        __builtin_amdgcn_sched_barrier(0);
        chirpz_inverse<R, TCH>(v, wscr, wscr_lds, tw, bw, fa, fb, ln, tid & 63);
        wave_lds_fence();
        put_line<R, H>(rowa, pa, ln);
        put_line<R, H>(rowa + CSN, v, ln);
        __builtin_amdgcn_sched_barrier(0);
        load_line(nitem, 1, vnb);                           // (needed a whole transform from now)
        __builtin_amdgcn_sched_barrier(0);
        lds_barrier();
        store_tile_transposed<BL, NT, NH, CSN>(job, tile, img, lb * BL, tid, N);
        lds_barrier();
    }
}

// The same for lines of 513..1024 points on the 2048-point wave-per-line FFT (tables of rowTB2_pass_kernel): one wave per line,
// 8 lines per workgroup, 64-byte runs in the transposed store.
struct IfftTB2Lds : IfftCzLds<2048 + 64, 1024> {
    static constexpr int M = 2048, NH = M / 2, NT = 512;
    static constexpr int W64 = TW + M;                            // tw: 2048, lane order (lds_pos64); then W_64
    static constexpr int LINES = NT / 64;                         // lines per work item: one per wave
    static constexpr int RS = (32 * W2K_PITCH) / 2 + 1;           // tile row pitch: a row is also its wave's transpose scratch
    static constexpr size_t bytes = (size_t)(TILE + LINES * RS) * sizeof(float2);
    static_assert(bytes <= IFFT_LDS_MAX, "ifftTB2_kernel: LDS");
};

__global__ void __launch_bounds__(512, 2) ifftTB2_kernel(IfftJob job) {
    using Lds = IfftTB2Lds;
    constexpr int R = 32, H = 16, NH = Lds::NH, LINES = Lds::LINES, NT = Lds::NT, RS = Lds::RS, TCH = 8;
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    float2* tw = reinterpret_cast<float2*>(smem_raw) + Lds::TW;
    float2* w64 = reinterpret_cast<float2*>(smem_raw) + Lds::W64;
    float2* bf = reinterpret_cast<float2*>(smem_raw) + Lds::BF;
    float2* bw = reinterpret_cast<float2*>(smem_raw) + Lds::BW;
    float2* tile = reinterpret_cast<float2*>(smem_raw) + Lds::TILE;
    const int tid = threadIdx.x;
    const int N = job.n_line;
    stage_wave2k_tables<NT>(tw, w64, job, tid);
    stage_table<NT>(bf, job.bf, NH + 1, tid);
    stage_table<NT>(bw, job.bw, NH, tid);
    __syncthreads();
    const int wv = tid >> 6, L = tid & 63, la = lam64(L);
    const float sgn = (L & 1) ? -1.f : 1.f;
    float2* myrow = tile + wv * RS;
    float* scr = reinterpret_cast<float*>(myrow);
    const float2* fa = bf + la;
    const float2* fb = bf - la;
    const int lblocks = (job.n_lines + LINES - 1) / LINES;
    const int n_items = lblocks * job.n_images;
    float2 vn[H];
    auto load_line = [&](int it) {
        const int img = it / lblocks, lb = it - img * lblocks;
        load_elements<64, H, true>(vn, in_line(job, img, min(lb * LINES + wv, job.n_lines - 1)), la, N, mirror_point(job, N));
    };
    if ((int)blockIdx.x < n_items) load_line(blockIdx.x);
    for (int item = blockIdx.x; item < n_items; item += gridDim.x) {
        const int img = item / lblocks, lb = item - img * lblocks;
        const int Lc = min(lb * LINES + wv, job.n_lines - 1);
        float2 v[R];
#pragma unroll
        for (int j = 0; j < H; ++j) v[j] = vn[j];
        __builtin_amdgcn_sched_barrier(0);
        if (item + (int)gridDim.x < n_items) load_line(item + (int)gridDim.x);
        __builtin_amdgcn_sched_barrier(0);
        mul_chirp<64, TCH>(v, bw, la);
        fft2048_wave<false, TCH>(v, scr, tw, w64, L, la, sgn);
        mul_filter<64, TCH>(v, fa, fb);
        fft2048_wave<true, TCH>(v, scr, tw, w64, L, la, sgn);
        mul_chirp<64, TCH>(v, bw, la);
        if (job.potential) apply_transmission<H>(job, v);
        if (stored_as_rows(job, img)) {
            if (lb * LINES + wv < job.n_lines) put_line<64, H, 0, true>(out_row(job, img, Lc), v, la, N);
            continue;
        }
        wave_lds_fence();
        put_line<64, H>(myrow, v, la);
        lds_barrier();
        store_tile_transposed<LINES, NT, NH, RS>(job, tile, img, lb * LINES, tid, N);
        lds_barrier();
    }
}

// ---- 2048-point axes: one wave per line on fft2048_wave, stored transposed through an 8-line tile (64-byte runs) ---------------
// (ifftT2_kernel<32>, the 2 R^2 layout with 64 complex per lane, spills and lost to the generic LDS kernel, which this one replaces.)
struct IfftTWLds {
    static constexpr int N = 2048, NT = 512;
    static constexpr int LINES = NT / 64;                         // lines per work item: one per wave
    static constexpr int LINE_BLOCK = LINES;                      // no guards: the line count is a multiple of it
    static constexpr int RS = N + 1;                              // tile row pitch
    static constexpr int TW = 0, W64 = TW + N, TILE = W64 + 64;   // tw: 2048, lane order; W_64; the tile
    static constexpr size_t bytes = (size_t)(TILE + LINES * RS) * sizeof(float2);
    static_assert(bytes <= IFFT_LDS_MAX, "ifftTW_kernel: LDS");
};

__global__ void __launch_bounds__(512, 2) ifftTW_kernel(IfftJob job) {
    using Lds = IfftTWLds;
    constexpr int R = 32, N = Lds::N, LINES = Lds::LINES, NT = Lds::NT, RS = Lds::RS;
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    float2* tw = reinterpret_cast<float2*>(smem_raw) + Lds::TW;
    float2* w64 = reinterpret_cast<float2*>(smem_raw) + Lds::W64;
    float2* tile = reinterpret_cast<float2*>(smem_raw) + Lds::TILE;
    const int tid = threadIdx.x;
    stage_wave2k_tables<NT>(tw, w64, job, tid);
    __syncthreads();
    const int wv = tid >> 6, L = tid & 63, la = lam64(L);
    const float sgn = (L & 1) ? -1.f : 1.f;
    float2* myrow = tile + wv * RS;
    float* scr = reinterpret_cast<float*>(myrow);
    const int lblocks = job.n_lines / LINES;
    const int n_items = lblocks * job.n_images;
    for (int item = blockIdx.x; item < n_items; item += gridDim.x) {      // (no register prefetch: 64 + 64 registers plus the transform spill)
        const int img = item / lblocks, lb = item - img * lblocks;
        float2 v[R];
        load_elements<64, R, false>(v, in_line(job, img, lb * LINES + wv), la, N, mirror_point(job, N));
        fft2048_wave<true, 8>(v, scr, tw, w64, L, la, sgn);
        if (job.potential) apply_transmission<R>(job, v);
        if (stored_as_rows(job, img)) {
            float2* dst = out_row(job, img, lb * LINES + wv);  // (spelled out: through put_line the kernel is scheduled on 194 registers, not 240)
#pragma unroll
            for (int j = 0; j < R; ++j) dst[j * 64 + la] = v[j];
            continue;
        }
        wave_lds_fence();
        put_line<64, R>(myrow, v, la);
        lds_barrier();
        store_tile_transposed<LINES, NT, N, RS, false>(job, tile, img, lb * LINES, tid);
        lds_barrier();
    }
}

}  // namespace msl
