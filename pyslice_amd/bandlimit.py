"""Band limit (anti-aliasing) of the slice loop (not in the reference, which applies none: SURVEY quirk Q8).

Every product t_k psi on an n-point grid folds the frequencies beyond Nyquist back into the pattern.  The cure of every multislice
code (Kirkland, abTEM, Dr. Probe, Prismatic) is to limit both factors to 2/3 of Nyquist.  Here the limit is a rectangle,

    M(kx, ky) = m_x(kx) m_y(ky),    m_d[h] = 1 for |h| <= c_d, else 0        (h = the signed FFT frequency index of the axis)

separable and even, so that it goes into the separable propagator tables and leaves the slice-loop kernels alone, with the same
physical cutoff on both axes: kc = fraction * min(1 / (2 dx), 1 / (2 dy)), and axis d keeps h iff |h| / (n_d d_d) < kc.

Alias-freeness per axis: the wave is confined to |h| <= c and the transmission function to |h| <= c, with 3 c < n.  Their product
reaches |h| <= 2 c, its fold-back lands at |h| >= n - 2 c > c, and the next propagator zeroes it.

The device masks the propagator tables and low-passes every transmission stack itself (msl_set_bandlimit, csrc/propagator.h,
csrc/bandlimit.h); `bandlimit_transmission` and `propagate_bandlimited` below are the float64 NumPy statement of the same run, which
the tests compare against.
"""
from __future__ import annotations

import math

import numpy as np

from .tilt import as_tilt, tilted_propagator

MAX_FRACTION = 2.0 / 3.0


class BandLimit:
    """MultisliceCalculator(bandlimit=BandLimit(fraction)) / Propagate(..., bandlimit=): keep the spatial frequencies below
    kc = fraction * min(1 / (2 dx), 1 / (2 dy)) (Angstrom^-1: isotropic in physical units) along each axis, in the propagator and in
    the transmission functions.  0 < fraction <= 2/3, anything else is a ValueError: above 2/3 the run would not be alias-free."""

    __slots__ = ("fraction",)

    def __init__(self, fraction=MAX_FRACTION):
        if isinstance(fraction, (bool, np.bool_)) or not isinstance(fraction, (int, float, np.integer, np.floating)) \
                or not math.isfinite(fraction) or not (0.0 < fraction <= MAX_FRACTION):
            raise ValueError(f"BandLimit: fraction must lie in (0, 2/3] (of Nyquist; above 2/3 the run is not alias-free), got {fraction!r}")
        object.__setattr__(self, "fraction", float(fraction))

    def __setattr__(self, name, value):
        raise AttributeError("BandLimit is immutable")

    def cutoff(self, dx, dy):
        """kc in Angstrom^-1"""
        return self.fraction * min(1.0 / (2.0 * dx), 1.0 / (2.0 * dy))

    def cuts(self, nx, ny, dx, dy):
        """(cx, cy): the largest kept |h| per axis, h kept iff |h| / (n d) < kc (strict, float64), and never beyond the alias-free
        bound 3 c < n (asserted).  The bound needs its own line: at fraction = 2/3 on the tighter axis of a length divisible by 3,
        h = n / 3 sits on the edge in exact arithmetic, and the float64 comparison can fall either way -- dx = 0.11 keeps
        h = 49 of 147 points, 51 of 153, 98 of 294 -- so such a cut is taken back to the largest h with 3 h < n, which is what the
        strict test means there.  ValueError when an axis keeps nothing but h = 0."""
        kc = self.cutoff(dx, dy)
        out = []
        for n, d in ((int(nx), float(dx)), (int(ny), float(dy))):
            c = int(math.floor(kc * n * d))
            while c > 0 and not (c / (n * d) < kc):
                c -= 1
            while (c + 1) / (n * d) < kc:
                c += 1
            c = min(c, (n - 1) // 3)                        # (the float64 edge at n / 3: see above)
            if c < 1:
                raise ValueError(f"BandLimit: fraction {self.fraction:g} keeps no frequency but zero along an axis of {n} points")
            assert 3 * c < n
            out.append(c)
        return tuple(out)

    def max_angle_mrad(self, wavelength, nx, ny, dx, dy):
        """the largest scattering angle kept along the tighter axis, in mrad: detectors and apertures inside it see no masked bin"""
        cx, cy = self.cuts(nx, ny, dx, dy)
        return 1e3 * wavelength * min(cx / (nx * dx), cy / (ny * dy))

    def __eq__(self, other):
        return isinstance(other, BandLimit) and self.fraction == other.fraction

    def __hash__(self):
        return hash(self.fraction)

    def __repr__(self):
        return f"BandLimit(fraction={self.fraction:g})"


def as_bandlimit(value, what="bandlimit"):
    """None, a BandLimit or a fraction of Nyquist -> None or a BandLimit"""
    if value is None or isinstance(value, BandLimit):
        return value
    if isinstance(value, (int, float, np.integer, np.floating)) and not isinstance(value, (bool, np.bool_)):
        return BandLimit(value)
    raise ValueError(f"{what}: expected a BandLimit object, a fraction of Nyquist or None, got {value!r}")


def mask_1d(n, c):
    """(n,) float64 of 0 / 1 in FFT order: 1 where the signed frequency index has |h| <= c (even in h)"""
    h = np.rint(np.fft.fftfreq(n) * n).astype(np.int64)
    return (np.abs(h) <= c).astype(np.float64)


def mask(nx, ny, cx, cy):
    """(nx, ny) float64 of 0 / 1 in FFT order: mask_1d(nx, cx) x mask_1d(ny, cy)"""
    return mask_1d(nx, cx)[:, None] * mask_1d(ny, cy)[None, :]


def bandlimit_transmission(t, cx, cy):
    """ifft2(mask * fft2(t_k)) of every slice of t (nz, nx, ny) or one slice (nx, ny), complex128"""
    t = np.asarray(t, dtype=np.complex128)
    m = mask(t.shape[-2], t.shape[-1], cx, cy)
    return np.fft.ifft2(m * np.fft.fft2(t, axes=(-2, -1)), axes=(-2, -1))


def propagate_bandlimited(psi0, transmission, dx, dy, wavelength, dz, cuts, tilt=None):
    """The slice loop in float64 under a band limit: psi0 (P, nx, ny) or (nx, ny) incident waves, transmission (nz, nx, ny) complex
    (slice-major, the UNLIMITED exp(i sigma V) of every slice) -> exit waves (P, nx, ny) complex128.  The recursion is the
    reference's (the test oracle's `propagate`; tilt.propagate_tilted) -- nz transmissions, nz - 1 propagations -- with two
    substitutions:
        P -> P * mask(cuts)                      (P = tilt.tilted_propagator: a tilt with a limit is a masked tilted table)
        t_k -> bandlimit_transmission(t_k)
    cuts = (cx, cy) from BandLimit.cuts(), or None for the plain recursion.

    The incident wave psi0 is NOT masked: it meets t_0 in full, and what the product carries beyond the band is removed by the
    first propagator.  The last operation of the recursion is a transmission, not a propagation: the exit wave is
    bandlimit(t_{nz-1}) times a wave confined to the band, so the exit spectrum is NOT zero outside the band.  Inside the band
    (|h| <= c) it is alias-free; beyond it, up to |h| <= 2 c, it holds the true product terms (of the two limited factors only),
    and from |h| >= n - 2 c on their fold-back.  A detector that is to see alias-free intensity only lies inside
    BandLimit.max_angle_mrad().  (The package does not import the oracle, which is test infrastructure; tests/test_bandlimit_host.py
    pins this recursion to the oracle's to 1e-12 where nothing is out of band.)"""
    psi = np.array(psi0, dtype=np.complex128)
    if psi.ndim == 2:
        psi = psi[None]
    t = np.asarray(transmission)
    if t.ndim != 3 or t.shape[1:] != psi.shape[1:]:
        raise ValueError(f"propagate_bandlimited: transmission {t.shape} does not match the waves {psi.shape}: expected (nz, nx, ny)")
    nz, nx, ny = t.shape
    prop = tilted_propagator(nx, ny, dx, dy, wavelength, dz, as_tilt(tilt))
    if cuts is not None:
        cx, cy = cuts
        if 3 * cx >= nx or 3 * cy >= ny or cx < 1 or cy < 1:
            raise ValueError(f"propagate_bandlimited: cuts {cuts} are not alias-free on the {nx} x {ny} grid (1 <= c, 3 c < n)")
        prop = prop * mask(nx, ny, cx, cy)
        t = bandlimit_transmission(t, cx, cy)
    for z in range(nz):
        psi = t[z][None] * psi
        if z < nz - 1:
            psi = np.fft.ifft2(prop[None] * np.fft.fft2(psi, axes=(-2, -1)), axes=(-2, -1))
    return psi
