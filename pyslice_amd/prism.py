"""PRISM (Ophus 2017): STEM exit waves from a plane-wave S-matrix (not in the reference, which propagates every probe position).

The multislice operator is linear in the incident wave and the engine applies no band limit in the propagator, so a probe is
a sum of plane waves, one per reciprocal-lattice point inside the aperture:

    beams    the unshifted pixels (mx, my) with signed indices h = fftfreq order, k = h / (n d), that satisfy
             hx % fx == 0, hy % fy == 0 and sqrt(kx^2 + ky^2) < mrad * 1e-3 / lambda (strict: the probe's own rule),
             in row-major order of (mx, my)
    S_b      = Propagate(pw_b),  pw_b[i, j] = exp(2 pi i (hx i / nx + hy j / ny))      (numpy's ifft2 basis function x nx ny)
    c[p, b]  = (fx fy / (nx ny)) exp(2 pi i [hx (floor(nx/2)/nx + px/Lx) + hy (floor(ny/2)/ny + py/Ly)]) exp(-i chi(k_b))
    psi_p(r) = W_p(r) sum_b c[p, b] S_b(r)

with W_p = 1 on the (nx/fx) x (ny/fy) periodic window centred on the pixel where the probe peaks (window_centre) and 0
elsewhere.  At interpolation (1, 1) W = 1 and psi_p IS the multislice exit wave of probe p; at f > 1 PRISM approximates the
physics (the probe tails outside the window are dropped and the beams are thinned), not the arithmetic.  The device builds S
with one slice loop per beam and frame (msl_smatrix_build) and every probe batch as one skinny complex GEMM
(msl_smatrix_probes); `prism_waves` below is the float64 NumPy statement of the same formula, which the tests compare against.

Prism(f, crop=True) synthesises the probes on PRISM's own (nx/fx) x (ny/fy) grid (msl_smatrix_probes_cropped).  The window of
probe p along x is wx = nx/fx consecutive pixels modulo nx and wx divides nx, so i -> i mod wx maps it one-to-one onto [0, wx).
Fold the windowed wave that way, psi_c[i mod wx, j mod wy] = psi_p[i, j] for (i, j) inside W_p (`prism_waves_cropped`); then

    fft2(psi_c)[m, n] = fft2(psi_p)[fx m, fy n]

exactly, with no phase ramp, because exp(-2 pi i m (i mod wx) / wx) = exp(-2 pi i (fx m) i / nx).  In stored (fftshifted) order
the cropped pixel (a, b) is the full pixel (nx//2 + fx (a - wx//2), ny//2 + fy (b - wy//2)) (`crop_index`): the cropped spectrum
is the full-grid one at every (fx, fy)-th pixel, value for value.  Nothing is rescaled: a sum over a region of the cropped
pattern is about 1 / (fx fy) of the uncropped run's sum over the same region, each cropped pixel standing for fx fy full pixels.
"""
from __future__ import annotations

import numpy as np


class Prism:
    """MultisliceCalculator(prism=Prism(interpolation)): interpolation = f or (fx, fy), positive integers that divide the grid
    (checked in setup()).  Prism(1) reproduces the multislice run from Bm slice loops per frame instead of one per probe.
    crop=True: every probe is synthesised, transformed and reduced on the cropped (nx / fx) x (ny / fy) grid -- the results are
    the uncropped run's spectra at the pixels crop_index names, not rescaled, on that grid's own k axes (.prism_crop = (fx, fy));
    at interpolation (1, 1) there is nothing to crop and the run is the one of crop=False."""

    def __init__(self, interpolation=1, crop=False):
        f = interpolation
        if isinstance(f, (bool, np.bool_)):
            raise ValueError(f"Prism: interpolation must be a positive integer or a pair of them, got {f!r}")
        if isinstance(f, (int, np.integer)):
            f = (f, f)
        try:
            f = tuple(f)
        except TypeError:
            raise ValueError(f"Prism: interpolation must be a positive integer or a pair of them, got {interpolation!r}") from None
        if len(f) != 2 or any(isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)) or int(v) < 1 for v in f):
            raise ValueError(f"Prism: interpolation must be a positive integer or a pair of them, got {interpolation!r}")
        if not isinstance(crop, (bool, np.bool_)):
            raise ValueError(f"Prism: crop must be True or False, got {crop!r}")
        self.interpolation = (int(f[0]), int(f[1]))
        self.crop = bool(crop)

    @property
    def cropped(self):
        """does a run with this object use the cropped grid?  (crop=True at interpolation (1, 1) runs as crop=False)"""
        return self.crop and self.interpolation != (1, 1)

    def __repr__(self):
        return f"Prism(interpolation={self.interpolation}, crop={self.crop})"


def signed_freq(n):
    """(n,) int64: the signed index of every unshifted pixel (numpy's fftfreq order)"""
    m = np.arange(n, dtype=np.int64)
    return np.where(m < (n + 1) // 2, m, m - n)


def beams(nx, ny, dx, dy, mrad, wavelength, f=(1, 1)):
    """(Bm, 2) int32 signed indices (hx, hy) of the beams of aperture `mrad` at interpolation f, in row-major order of the
    unshifted pixels -- the order of the S-matrix (msl_smatrix_beams)"""
    fx, fy = int(f[0]), int(f[1])
    if not mrad > 0:
        raise ValueError("beams: the aperture must be positive")
    if fx < 1 or fy < 1 or nx % fx or ny % fy:
        raise ValueError(f"beams: interpolation ({fx}, {fy}) must be positive and divide the {nx} x {ny} grid")
    hx, hy = signed_freq(nx), signed_freq(ny)
    kx = hx * (1.0 / (nx * dx))                      # fftfreq value = index * (1 / (n d)), as the probe kernel
    ky = hy * (1.0 / (ny * dy))
    keep = np.sqrt(kx[:, None] ** 2 + ky[None, :] ** 2) < (mrad * 1e-3) / wavelength
    keep &= (hx % fx == 0)[:, None] & (hy % fy == 0)[None, :]
    ix, iy = np.nonzero(keep)                        # row-major
    return np.stack([hx[ix], hy[iy]], axis=1).astype(np.int32)


def window_centre(n, d, p):
    """the pixel where the engine's probe at position p (Angstrom) peaks along an axis of n pixels of size d: the reference's
    ramp exp(+2 pi i k p) puts the probe at centre - p"""
    return int((-(n // 2) - int(np.rint(p / d))) % n)


def window_mask(n, d, p, f):
    """(n,) bool: the periodic window of n // f pixels centred on window_centre(n, d, p)"""
    w = n // f
    return ((np.arange(n) - window_centre(n, d, p) + w // 2) % n) < w


def plane_waves(nx, ny, hxhy):
    """(Bm, nx, ny) complex128: pw_b[i, j] = exp(2 pi i (hx i / nx + hy j / ny))"""
    hxhy = np.asarray(hxhy, dtype=np.int64).reshape(-1, 2)
    i, j = np.arange(nx, dtype=np.int64), np.arange(ny, dtype=np.int64)
    ax = np.exp(2j * np.pi * ((hxhy[:, 0:1] * i[None, :]) % nx) / nx)
    ay = np.exp(2j * np.pi * ((hxhy[:, 1:2] * j[None, :]) % ny) / ny)
    return ax[:, :, None] * ay[:, None, :]


def coefficients(hxhy, xy, nx, ny, dx, dy, f=(1, 1), wavelength=None, aberrations=None):
    """(P, Bm) complex128: c[p, b] of the definition above"""
    hxhy = np.asarray(hxhy, dtype=np.float64).reshape(-1, 2)
    xy = np.asarray(xy, dtype=np.float64).reshape(-1, 2)
    t = (hxhy[None, :, 0] * ((nx // 2) / nx + xy[:, 0:1] / (nx * dx)) + hxhy[None, :, 1] * ((ny // 2) / ny + xy[:, 1:2] / (ny * dy)))
    c = (f[0] * f[1] / (nx * ny)) * np.exp(2j * np.pi * t)
    if aberrations is not None and not aberrations.is_zero:
        if wavelength is None:
            raise ValueError("coefficients: aberrations need the wavelength")
        chi = aberrations.chi(hxhy[:, 0] / (nx * dx), hxhy[:, 1] / (ny * dy), wavelength)
        c = c * np.exp(-1j * chi)[None, :]
    return c


def prism_waves(S, hxhy, xy, dx, dy, f=(1, 1), wavelength=None, aberrations=None):
    """(P, nx, ny) complex128: psi_p = W_p sum_b c[p, b] S_b for the S-matrix S (Bm, nx, ny), its beams hxhy (Bm, 2) and the
    probe positions xy (P, 2) in Angstrom -- the definition of what msl_smatrix_probes computes, in float64"""
    S = np.asarray(S)
    Bm, nx, ny = S.shape
    xy = np.asarray(xy, dtype=np.float64).reshape(-1, 2)
    c = coefficients(hxhy, xy, nx, ny, dx, dy, f, wavelength, aberrations)
    out = np.tensordot(c, S.astype(np.complex128, copy=False), axes=(1, 0))
    for p, (px, py) in enumerate(xy):
        out[p] *= window_mask(nx, dx, px, int(f[0]))[:, None] & window_mask(ny, dy, py, int(f[1]))[None, :]
    return out


def crop_index(n, f):
    """(n // f,) int64: the stored (fftshifted) full-grid index of every stored pixel of the cropped axis, n//2 + f (a - (n//f)//2)
    -- the DC pixel maps to the DC pixel, and every index exists for odd and even lengths alike"""
    n, f = int(n), int(f)
    if f < 1 or n % f:
        raise ValueError(f"crop_index: the interpolation {f} must be positive and divide the axis of {n} pixels")
    w = n // f
    return n // 2 + f * (np.arange(w, dtype=np.int64) - w // 2)


def prism_waves_cropped(S, hxhy, xy, dx, dy, f=(1, 1), wavelength=None, aberrations=None):
    """(P, nx // fx, ny // fy) complex128: prism_waves folded onto the cropped grid, psi_c[i mod wx, j mod wy] = psi_p[i, j] for
    (i, j) inside the window of probe p (one-to-one: the window is wx consecutive pixels modulo nx and wx divides nx) -- the
    definition of what msl_smatrix_probes_cropped computes, in float64.  fft2(psi_c) == fft2(psi_p)[::fx, ::fy]."""
    full = prism_waves(S, hxhy, xy, dx, dy, f, wavelength, aberrations)
    P, nx, ny = full.shape
    fx, fy = int(f[0]), int(f[1])
    wx, wy = nx // fx, ny // fy
    xy = np.asarray(xy, dtype=np.float64).reshape(-1, 2)
    out = np.zeros((P, wx, wy), dtype=np.complex128)
    for p, (px, py) in enumerate(xy):
        ix = np.nonzero(window_mask(nx, dx, px, fx))[0]
        iy = np.nonzero(window_mask(ny, dy, py, fy))[0]
        out[p][np.ix_(ix % wx, iy % wy)] = full[p][np.ix_(ix, iy)]
    return out
