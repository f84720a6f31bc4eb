// The slice loop backwards (pyslice_amd/adjoint.py is the definition): for a data-fit loss L of the exit
// patterns I = |Psi|^2 against measured patterns D, the derivative with respect to the slice potentials,
//     dL/dV_s(r) = 2 sigma sum_p Im( g_p,s(r) conj(phi_p,s(r)) ),     phi_p,s = t_s psi_p,s,
// with the adjoint wave g: g = N ifft2(G) at the exit, G = dL/dPsi* the residual, then per slice g <- conj(t_s) g and, for s > 0,
// g <- ifft2(conj(P) fft2 g).  The kernels here: the residual pass over the exit spectra, the per-slice step, and the conjugate
// propagator between the two transforms of fft2_inplace.  The waves psi_s are the forward loop's, kept by its store hook.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "aberration.h"

namespace msl {

enum AdjointLoss { ADJ_OFF = 0, ADJ_AMPLITUDE = 1, ADJ_INTENSITY = 2, ADJ_POISSON = 3 };

constexpr int ADJ_RES_PER = 4, ADJ_RES_TILE = 256 * ADJ_RES_PER;       // pixels per lane and per tile of the residual pass
constexpr int ADJ_SL = 2, ADJ_TILE = 256 * ADJ_SL;                     // pixel pairs per lane and per tile of the step

// The residual pass.  spec: (B, nx, pitch) c64, the exit spectra Psi in the transform's own order, rewritten in place with G; D:
// (B, nx, ny) f32 and w: (nx, ny) f32 or null, both in the detector's layout (fftshifted: detector pixel i holds frequency index
// (i - n / 2) mod n), which the index maps -- no shift pass.  A workgroup owns tile blockIdx.x of the nx * ny pixels of image
// blockIdx.y; the loss terms are formed and summed in float64 (lane, wave by shuffles, the four waves through the LDS in wave
// order) and thread 0 stores part[tile * B + image].  No atomics: the same input gives the same bits.
template <int LOSS>
__global__ void __launch_bounds__(256) adjoint_residual_kernel(float2* __restrict__ spec, const float* __restrict__ D, const float* __restrict__ w,
                                                               int nx, int ny, int pitch, int B, float eps, double* __restrict__ part) {
    __shared__ double lds[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int p = blockIdx.y;
    const long long npix = (long long)nx * ny;
    float2* img = spec + (long long)p * nx * pitch;
    const float* Dp = D + (long long)p * npix;
    const float sqrt_eps = sqrtf(eps);
    double loss = 0.0;
#pragma unroll
    for (int s = 0; s < ADJ_RES_PER; ++s) {
        const long long q = (long long)blockIdx.x * ADJ_RES_TILE + (long long)s * 256 + threadIdx.x;
        if (q >= npix) continue;
        const int x = (int)(q / ny), y = (int)(q - (long long)x * ny);
        int xs = x + nx / 2, ys = y + ny / 2;               // the detector pixel of frequency index (x, y)
        if (xs >= nx) xs -= nx;
        if (ys >= ny) ys -= ny;
        const long long k = (long long)xs * ny + ys;
        const float d = Dp[k], wk = w ? w[k] : 1.f;
        const float2 v = img[(long long)x * pitch + y];
        const float I = v.x * v.x + v.y * v.y;
        float f;                                            // G = f Psi
        if constexpr (LOSS == ADJ_AMPLITUDE) {
            const float a = sqrtf(I), sd = sqrtf(d);
            f = wk * (1.f - sd / fmaxf(a, sqrt_eps));
            const double r = (double)a - (double)sd;
            loss += (double)wk * r * r;
        } else if constexpr (LOSS == ADJ_INTENSITY) {
            f = wk * (I - d);
            const double r = (double)I - (double)d;
            loss += 0.5 * (double)wk * r * r;
        } else {
            f = wk * (1.f - d / (I + eps));
            loss += (double)wk * ((double)I - (double)d * log((double)I + (double)eps));
        }
        img[(long long)x * pitch + y] = make_float2(f * v.x, f * v.y);
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) loss += __shfl_xor(loss, o, 64);
    if (lane == 0) lds[wave] = loss;
    __syncthreads();
    if (threadIdx.x == 0) part[(long long)blockIdx.x * B + p] = ((lds[0] + lds[1]) + lds[2]) + lds[3];
}

// The step of slice s.  g: (B, nx, pitch) c64, the adjoint waves behind slice s, rewritten with conj(t_s) g; psi: (B, nx, pitch) c64,
// the waves psi_s arriving at the slice; t: (nx, ny) c64, t_s; grad: (nx, ny) float64, row s of the accumulator.  The pixels of an
// image are taken in pairs along y as slice_sums_kernel takes them (ppr = (ny + 1) / 2 pairs per row; the second pixel of the last
// pair of an odd row does not exist): a workgroup owns tile blockIdx.x, loads t_s of its pairs once into registers and streams all B
// images of g and psi through them with the next image's loads in flight.  Per image phi = t psi, Im(g conj phi) is added into the
// lane's f32 sum in image order, and conj(t) g is stored.  At the end the lane adds 2 sigma x its sums to its pixels of grad: a plain
// load, add and store -- a pixel has one owner and the batches are serial on the stream, so no atomics and the same bits every run.
// VEC: pitch even and g, psi on 16 bytes -- one 16-byte access per pair (an odd row's last pair loads its pad pixel and drops it,
// and stores 8 bytes); else 8-byte accesses.
template <bool VEC>
__global__ void __launch_bounds__(256) adjoint_step_kernel(float2* __restrict__ g, const float2* __restrict__ psi, const float2* __restrict__ t,
                                                           int nx, int ny, int pitch, int B, double two_sigma, double* __restrict__ grad) {
    constexpr int SL = ADJ_SL;
    const int ppr = (ny + 1) >> 1;
    const long long pairs = (long long)nx * ppr;
    const long long image_stride = (long long)nx * pitch;

    long long off[SL];                  // element offset of the pair inside an image, -1: no such pair
    long long pix[SL];                  // its first pixel in the dense (nx, ny) images
    bool two[SL];                       // the pair has its second pixel
    float4 tt[SL];
    float acc[SL][2];
#pragma unroll
    for (int s = 0; s < SL; ++s) {
        const long long q = (long long)blockIdx.x * ADJ_TILE + (long long)s * 256 + threadIdx.x;
        off[s] = -1; pix[s] = 0; two[s] = false;
        tt[s] = make_float4(0.f, 0.f, 0.f, 0.f);
        acc[s][0] = acc[s][1] = 0.f;
        if (q < pairs) {
            const int x = (int)(q / ppr), y = 2 * (int)(q - (long long)x * ppr);
            off[s] = (long long)x * pitch + y;
            pix[s] = (long long)x * ny + y;
            two[s] = y + 1 < ny;
            const float2 a = t[pix[s]];
            tt[s].x = a.x; tt[s].y = a.y;
            if (two[s]) { const float2 b = t[pix[s] + 1]; tt[s].z = b.x; tt[s].w = b.y; }
        }
    }

    auto load = [&](const float2* img, float4 (&v)[SL]) {
#pragma unroll
        for (int s = 0; s < SL; ++s) {
            v[s] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (off[s] < 0) continue;
            if constexpr (VEC) {
                const float4 r = *reinterpret_cast<const float4*>(img + off[s]);     // (a pad pixel behind an odd row is read and dropped)
                v[s].x = r.x; v[s].y = r.y;
                if (two[s]) { v[s].z = r.z; v[s].w = r.w; }
            } else {
                const float2 a = img[off[s]];
                v[s].x = a.x; v[s].y = a.y;
                if (two[s]) { const float2 b = img[off[s] + 1]; v[s].z = b.x; v[s].w = b.y; }
            }
        }
    };

    float4 gn[SL], pn[SL];
    if (B > 0) { load(g, gn); load(psi, pn); }
    for (int p = 0; p < B; ++p) {
        float4 gv[SL], pv[SL];
#pragma unroll
        for (int s = 0; s < SL; ++s) { gv[s] = gn[s]; pv[s] = pn[s]; }
        if (p + 1 < B) { load(g + (long long)(p + 1) * image_stride, gn); load(psi + (long long)(p + 1) * image_stride, pn); }
        float2* out = g + (long long)p * image_stride;
#pragma unroll
        for (int s = 0; s < SL; ++s) {
            if (off[s] < 0) continue;
            // phi = t psi; Im(g conj phi) = g.y phi.x - g.x phi.y; g <- conj(t) g
            const float f0x = tt[s].x * pv[s].x - tt[s].y * pv[s].y, f0y = tt[s].x * pv[s].y + tt[s].y * pv[s].x;
            const float f1x = tt[s].z * pv[s].z - tt[s].w * pv[s].w, f1y = tt[s].z * pv[s].w + tt[s].w * pv[s].z;
            acc[s][0] += gv[s].y * f0x - gv[s].x * f0y;
            acc[s][1] += gv[s].w * f1x - gv[s].z * f1y;
            const float o0x = tt[s].x * gv[s].x + tt[s].y * gv[s].y, o0y = tt[s].x * gv[s].y - tt[s].y * gv[s].x;
            const float o1x = tt[s].z * gv[s].z + tt[s].w * gv[s].w, o1y = tt[s].z * gv[s].w - tt[s].w * gv[s].z;
            if (VEC && two[s]) {
                *reinterpret_cast<float4*>(out + off[s]) = make_float4(o0x, o0y, o1x, o1y);
            } else {
                out[off[s]] = make_float2(o0x, o0y);
                if (two[s]) out[off[s] + 1] = make_float2(o1x, o1y);
            }
        }
    }
#pragma unroll
    for (int s = 0; s < SL; ++s) {
        if (off[s] < 0) continue;
        grad[pix[s]] = grad[pix[s]] + two_sigma * (double)acc[s][0];
        if (two[s]) grad[pix[s] + 1] = grad[pix[s] + 1] + two_sigma * (double)acc[s][1];
    }
}

// g(kx, ky) <- conj(px[kx] py[ky]) g(kx, ky) over B images (nx, pitch) between fft2_inplace(+1) and fft2_inplace(-1): px and py are the
// handle's own propagator tables, which carry its tilt and the 1 / nx and 1 / ny of the inverse transform
__global__ void __launch_bounds__(256) adjoint_conjprop_kernel(float2* __restrict__ g, const float2* __restrict__ px, const float2* __restrict__ py,
                                                               int nx, int ny, int pitch, long long total) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const long long row = i / ny;
    const int y = (int)(i - row * ny), x = (int)(row % nx);
    const float2 a = px[x], b = py[y];
    const float2 c = make_float2(a.x * b.x - a.y * b.y, -(a.x * b.y + a.y * b.x));      // conj(px py)
    float2* q = g + row * pitch + y;
    const float2 v = *q;
    *q = make_float2(c.x * v.x - c.y * v.y, c.x * v.y + c.y * v.x);
}

// ---- gradients with respect to atom positions: the potential build backwards ----
// With Gamma_s = dL/dV_s, B_s = fft2(Gamma_s) and c = 2 pi / (N dx^2 dy^2), for atom a of species Z in slice s
//     dL/dx_a = c sum_{mx, my} kx(mx) f_Z(mx, my) Im( conj(B_s(mx, my)) ex_a(mx) ey_a(my) ),     dL/dy_a: the same with ky(my),
// over the FULL grid of fftfreq indices -- the structure factor's sum over atoms x k-bins run the other way, gathering at the atoms.
// ex, ey are the sorted phase tables the build left (columns 0 .. n/2; a negative frequency m > n/2 is the conjugate of column n - m;
// on an even length column n/2 IS the grid's one Nyquist frequency -n/2, so no line is folded and none counts twice).

constexpr int PG_ATOMS = 8;                     // atoms (sorted table rows) per tile
constexpr int PG_ROWS = 256 / PG_ATOMS;         // kx rows whose x phases are staged in the LDS at a time: one entry per thread

// Gamma (n_images, nx, ny) float64 -> c64 images of pitch ny, imaginary part zero
__global__ void __launch_bounds__(256) position_gamma_kernel(const double* __restrict__ gamma, float2* __restrict__ img, long long total) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < total) img[i] = make_float2((float)gamma[i], 0.f);
}

// A workgroup owns tile blockIdx.x: rows a0 .. a0 + na - 1 (na <= PG_ATOMS) of the sorted tables, all of one (slice, species) bin --
// tiles[t] = (slice, species, a0, na).  Thread t owns the columns my = t, t + 256, ...; per column block it walks the rows mx of
// W = f_Z conj(B_s) once (coalesced along my), PG_ROWS at a time: the x phases of the tile's atoms at those rows, and kx times them,
// are staged in the LDS (every lane reads the same entry: a broadcast), and every loaded element of W feeds both components of all
// atoms of the tile -- eight FMAs per atom and element into per-lane f32 sums  sum_mx kx W ex  and  sum_mx W ex.  After each block
// of PG_ROWS rows the lane multiplies by its own ey_a(my) (and ky), takes the imaginary part and adds it into its float64 sums; at
// the end the float64 sums are combined over the lanes of a wave by shuffles and over the four waves through the LDS in wave
// order, scaled by c and stored to out[order[row]][ax1 / ax2] -- a row has one owner: no atomics, the same bits every run.  Padding
// rows of a bin (order < 0, zero phases) are computed and not stored.
// img: the images B_s of the slices s_base .. (pitch ny); kfx = 1 / (nx dx), kfy = 1 / (ny dy).
__global__ void __launch_bounds__(256) position_gradient_kernel(const int4* __restrict__ tiles, const float2* __restrict__ img, int s_base,
                                                                const float2* __restrict__ ex, const float2* __restrict__ ey,
                                                                const float* __restrict__ ff, const int* __restrict__ order, int nx, int ny,
                                                                int cx, int cy, float kfx, float kfy, double c, int ax1, int ax2,
                                                                double* __restrict__ out) {
    constexpr int TA = PG_ATOMS, RC = PG_ROWS;
    __shared__ float4 sh_ex[RC][TA];            // (ex, kx ex) of row r and atom a
    __shared__ double sh_red[4][TA][2];
    const int4 tile = tiles[blockIdx.x];
    const int s = tile.x, sp = tile.y, a0 = tile.z, na = tile.w;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int hx = nx / 2, hy = ny / 2;
    const float2* Bs = img + (size_t)(s - s_base) * nx * ny;
    const float* f = ff + (size_t)sp * nx * ny;
    double gx[TA], gy[TA];
#pragma unroll
    for (int a = 0; a < TA; ++a) { gx[a] = 0.0; gy[a] = 0.0; }
    for (int y0 = 0; y0 < ny; y0 += 256) {
        const int my = y0 + (int)threadIdx.x;
        const bool live = my < ny;
        const int col = my <= hy ? my : ny - my;
        const float kyw = live ? (float)(my < (ny + 1) / 2 ? my : my - ny) * kfy : 0.f;
        float2 eyv[TA];
#pragma unroll
        for (int a = 0; a < TA; ++a) {
            eyv[a] = make_float2(0.f, 0.f);
            if (live && a < na) {
                eyv[a] = ey[(size_t)(a0 + a) * cy + col];
                if (my > hy) eyv[a].y = -eyv[a].y;
            }
        }
        for (int x0 = 0; x0 < nx; x0 += RC) {
            __syncthreads();                                    // the readers of the previous block are done
            {
                const int r = threadIdx.x / TA, a = threadIdx.x % TA, mx = x0 + r;
                float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
                if (mx < nx && a < na) {
                    float2 e = ex[(size_t)(a0 + a) * cx + (mx <= hx ? mx : nx - mx)];
                    if (mx > hx) e.y = -e.y;
                    const float kxw = (float)(mx < (nx + 1) / 2 ? mx : mx - nx) * kfx;
                    v = make_float4(e.x, e.y, kxw * e.x, kxw * e.y);
                }
                sh_ex[r][a] = v;
            }
            __syncthreads();
            if (!live) continue;
            float px[TA][2], py[TA][2];                         // sum_mx kx W ex and sum_mx W ex of this block of rows
#pragma unroll
            for (int a = 0; a < TA; ++a) { px[a][0] = px[a][1] = 0.f; py[a][0] = py[a][1] = 0.f; }
            const int rows = min(RC, nx - x0);
            for (int r = 0; r < rows; ++r) {
                const size_t q = (size_t)(x0 + r) * ny + my;
                const float2 b = Bs[q];
                const float w = f[q];
                const float wr = w * b.x, wi = -(w * b.y);      // W = f conj(B)
#pragma unroll
                for (int a = 0; a < TA; ++a) {
                    const float4 e = sh_ex[r][a];
                    py[a][0] = fmaf(wr, e.x, fmaf(-wi, e.y, py[a][0]));
                    py[a][1] = fmaf(wr, e.y, fmaf(wi, e.x, py[a][1]));
                    px[a][0] = fmaf(wr, e.z, fmaf(-wi, e.w, px[a][0]));
                    px[a][1] = fmaf(wr, e.w, fmaf(wi, e.z, px[a][1]));
                }
            }
#pragma unroll
            for (int a = 0; a < TA; ++a) {                      // Im(p ey) = p.re ey.im + p.im ey.re
                gx[a] += (double)fmaf(px[a][0], eyv[a].y, px[a][1] * eyv[a].x);
                gy[a] += (double)(kyw * fmaf(py[a][0], eyv[a].y, py[a][1] * eyv[a].x));
            }
        }
    }
#pragma unroll
    for (int a = 0; a < TA; ++a) {
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) { gx[a] += __shfl_xor(gx[a], o, 64); gy[a] += __shfl_xor(gy[a], o, 64); }
    }
    __syncthreads();
    if (lane == 0) {
#pragma unroll
        for (int a = 0; a < TA; ++a) { sh_red[wave][a][0] = gx[a]; sh_red[wave][a][1] = gy[a]; }
    }
    __syncthreads();
    if (threadIdx.x < 2 * TA) {
        const int a = threadIdx.x >> 1, comp = threadIdx.x & 1;
        if (a < na) {
            const int atom = order[a0 + a];
            if (atom >= 0)
                out[(size_t)atom * 3 + (comp ? ax2 : ax1)] = c * (((sh_red[0][a][comp] + sh_red[1][a][comp]) + sh_red[2][a][comp]) + sh_red[3][a][comp]);
        }
    }
}

// ---- gradients with respect to scan positions and probe aberrations: the probe recipe backwards ----
// msl_set_probes builds psi0_p = ifft2(Phi_p), Phi_p(k) = A(k) exp(2 pi i (t_ramp,p(k) - chi(k) / 2 pi)) (probe_kspace_aberr_kernel).  With
// g0 = dL/dpsi0_p*, ghat = fft2(g0) (unnormalised) and the real field m_p(k) = Im(conj(ghat(k)) Phi_p(k)) over the aperture,
//     dL/dx_p = -(4 pi / N) sum_k kx m_p(k),     dL/da_j = +(4 pi / N) sum_k A_j(k) m_p(k)     (and ky, B_j likewise),
// A_j, B_j the factors of the coefficients in chi / 2 pi (aberration_basis).  The kernel forms the 27 sums without the factor: kx, ky, the
// fourteen A_j and the eleven B_j of the terms with m > 0, in that order (PM_SLOTS).

constexpr int PM_SLOTS = 27;
constexpr int PM_B_TERM[11] = {1, 2, 3, 5, 6, 7, 8, 9, 11, 12, 13};     // the terms with m > 0: slot 16 + k holds B of term PM_B_TERM[k]
constexpr int PM_PER = 4, PM_TILE = 256 * PM_PER;      // box pixels per lane and per tile

// the aperture's bounding box in wrapped index space: the signed frequencies lo .. lo + w - 1 of an axis
struct ProbeBox {
    int x_lo, wx, y_lo, wy;
};

// ghat: (B, nx, pitch) c64.  A workgroup owns tile blockIdx.x of the box's wx * wy pixels (rows of the box in order) of probe
// blockIdx.y; a lane takes PM_PER of them, recomputes Phi_p(k) in float64 as probe_kspace_aberr_kernel does (the same ramp, the same
// polynomial, the same reduction to one turn, the same aperture test; ab is all zero without aberrations) and adds m and its
// products with the basis into 27 float64 sums.  The sums are combined over a wave by shuffles and over the four waves through the
// LDS in wave order; part[(tile * B + probe) * 27 + slot].  No atomics: the same input gives the same bits.
__global__ void __launch_bounds__(256) probe_moment_kernel(const float2* __restrict__ ghat, const double* __restrict__ xy, int B, int nx, int ny,
                                                           int pitch, ProbeBox box, double inv_lx, double inv_ly, double kfreq_x, double kfreq_y,
                                                           double radius, double wavelength, ProbeAberrations ab, double* __restrict__ part) {
    __shared__ double lds[4][PM_SLOTS];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int p = blockIdx.y;
    const long long nbox = (long long)box.wx * box.wy;
    const float2* img = ghat + (long long)p * nx * pitch;
    const double px = xy[2 * p], py = xy[2 * p + 1];
    double acc[PM_SLOTS];
#pragma unroll
    for (int k = 0; k < PM_SLOTS; ++k) acc[k] = 0.0;
    for (int s = 0; s < PM_PER; ++s) {
        const long long q = (long long)blockIdx.x * PM_TILE + (long long)s * 256 + threadIdx.x;
        if (q >= nbox) continue;
        const int i = (int)(q / box.wy), j = (int)(q - (long long)i * box.wy);
        const int fx = box.x_lo + i, fy = box.y_lo + j;                 // signed frequency indices
        const int mx = fx < 0 ? fx + nx : fx, my = fy < 0 ? fy + ny : fy;
        const double kx = fx * kfreq_x, ky = fy * kfreq_y;
        if (!(sqrt(kx * kx + ky * ky) < radius)) continue;
        const double ax = wavelength * kx, ay = wavelength * ky;
        const AberrationPowers w = aberration_powers(ax, ay);
        double t = fx * ((double)(nx / 2) / nx + px * inv_lx) + fy * ((double)(ny / 2) / ny + py * inv_ly);
        t -= aberration_chi_turns(w, ax, ay, ab, ab.a[0]);
        t -= rint(t);
        double sn, cs;
        sincospi(2.0 * t, &sn, &cs);
        const float2 g = img[(long long)mx * pitch + my];
        const double m = (double)g.x * sn - (double)g.y * cs;          // Im(conj(ghat) Phi)
        double A[14], Bm[14];
        aberration_basis(w, A, Bm);
        acc[0] = fma(kx, m, acc[0]);
        acc[1] = fma(ky, m, acc[1]);
#pragma unroll
        for (int k = 0; k < 14; ++k) acc[2 + k] = fma(A[k], m, acc[2 + k]);
#pragma unroll
        for (int k = 0; k < 11; ++k) acc[16 + k] = fma(Bm[PM_B_TERM[k]], m, acc[16 + k]);
    }
#pragma unroll
    for (int k = 0; k < PM_SLOTS; ++k) {
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) acc[k] += __shfl_xor(acc[k], o, 64);
    }
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < PM_SLOTS; ++k) lds[wave][k] = acc[k];
    }
    __syncthreads();
    if (threadIdx.x < PM_SLOTS) {
        const int k = threadIdx.x;
        part[((long long)blockIdx.x * B + p) * PM_SLOTS + k] = ((lds[0][k] + lds[1][k]) + lds[2][k]) + lds[3][k];
    }
}

}  // namespace msl
