"""Objective lens of an imaging run (HRTEM, focal series): MultisliceCalculator(imaging=Imaging(...)).run_images().

For probe p, defocus index f, over the T frozen-phonon frames

    I[p, f](r) = (1/T) sum_t sum_i w_i | ifft2( ifftshift(Psi[p, t]) * H_{f,i} )(r) |^2
    H(k)       = A(k) exp(-i chi(k)),   A(k) = 1 if |k| < k_ap (strict, the probe's rule) or if no aperture is set, else 0

with Psi the stored exit spectrum fftshift(fft2(exit)), unnormalised, ifft2 NumPy's, and chi exactly Aberrations.chi: chi_{f,i} is the
objective's chi with C10 + defocus_series[f] + delta_i.

Sign of defocus: C10 = +dz gives exp(-i pi lambda dz k^2), the Fresnel factor of the slice loop and of the oracle's propagate().  An
image at defocus = +dz is therefore the intensity a distance dz DOWNSTREAM of the exit surface -- the OPPOSITE of abTEM, where
defocus = -C10 (as for the probe, aberrations.py).

Focal spread (temporal coherence) is the exact incoherent average over a Gaussian of standard deviation Delta, not an envelope:
Gauss-Hermite nodes delta_i = sqrt(2) Delta x_i with weights w_i = omega_i / sqrt(pi) from numpy.polynomial.hermite.hermgauss(N).

The device pass is msl_image_add (pyslice_amd/csrc/image.h); `Imaging.transfer` is the float64 NumPy statement of H the tests
compare against.  Not in the reference, which has no imaging mode.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Optional, Tuple

import numpy as np

from .aberrations import Aberrations


@dataclass(frozen=True)
class Imaging:
    """aberrations: the objective's Aberrations (None: none); aperture_mrad: objective aperture half-angle (None: no aperture);
    defocus_series: defocus values (Angstrom) ADDED to aberrations.C10, one image each; focal_spread: standard deviation Delta
    (Angstrom) of the defocus distribution; focal_points: odd number N of Gauss-Hermite nodes (N > 1 needs focal_spread > 0).
    Any non-finite number, an empty series, an even or non-positive N raises ValueError."""
    aberrations: Optional[Aberrations] = None
    aperture_mrad: Optional[float] = None
    defocus_series: Tuple[float, ...] = (0.0,)
    focal_spread: float = 0.0
    focal_points: int = 1

    def __post_init__(self):
        if self.aberrations is not None and not isinstance(self.aberrations, Aberrations):
            raise ValueError(f"Imaging: aberrations must be an Aberrations object, got {self.aberrations!r}")

        def number(name, v):
            try:
                v = float(v)
            except (TypeError, ValueError):
                raise ValueError(f"Imaging: {name} must be a number, got {v!r}") from None
            if not math.isfinite(v):
                raise ValueError(f"Imaging: {name} must be finite, got {v}")
            return v
        if self.aperture_mrad is not None:
            ap = number("aperture_mrad", self.aperture_mrad)
            if ap <= 0:
                raise ValueError(f"Imaging: aperture_mrad must be positive (None: no aperture), got {ap}")
            object.__setattr__(self, "aperture_mrad", ap)
        try:
            series = tuple(np.atleast_1d(np.asarray(self.defocus_series, dtype=object)).tolist())
        except Exception:
            raise ValueError(f"Imaging: defocus_series must be a sequence of numbers, got {self.defocus_series!r}") from None
        if len(series) == 0:
            raise ValueError("Imaging: defocus_series is empty")
        object.__setattr__(self, "defocus_series", tuple(number("defocus_series", v) for v in series))
        spread = number("focal_spread", self.focal_spread)
        if spread < 0:
            raise ValueError(f"Imaging: focal_spread must not be negative, got {spread}")
        object.__setattr__(self, "focal_spread", spread)
        n = self.focal_points
        if isinstance(n, (bool, np.bool_)) or not isinstance(n, (int, np.integer)) or int(n) < 1 or int(n) % 2 == 0:
            raise ValueError(f"Imaging: focal_points must be an odd integer >= 1, got {n!r}")
        if int(n) > 1 and spread == 0:
            raise ValueError("Imaging: focal_points > 1 needs focal_spread > 0")
        object.__setattr__(self, "focal_points", int(n))

    def nodes(self):
        """(delta_i, w_i): defocus offsets (Angstrom) and weights (sum 1) of the focal-spread average; one node (0, 1.0) when
        focal_points == 1 or focal_spread == 0"""
        if self.focal_points == 1 or self.focal_spread == 0:
            return np.array([0.0]), np.array([1.0])
        x, w = np.polynomial.hermite.hermgauss(self.focal_points)
        return math.sqrt(2.0) * self.focal_spread * x, w / math.sqrt(math.pi)

    def polar(self, f=0, i=0):
        """(14, 2) float64 of msl_image_add: the objective's coefficients with C10 + defocus_series[f] + delta_i"""
        p = self.aberrations.as_polar() if self.aberrations is not None else np.zeros((14, 2), dtype=np.float64)
        p = np.array(p, dtype=np.float64)
        p[0, 0] = (p[0, 0] + self.defocus_series[f]) + self.nodes()[0][i]
        return p

    def aperture_k(self, wavelength):
        """aperture radius in 1/Angstrom (0.0: no aperture)"""
        return 0.0 if self.aperture_mrad is None else (self.aperture_mrad * 1e-3) / wavelength

    def transfer(self, kx, ky, wavelength, f=0, i=0):
        """H(k) = A(k) exp(-i chi_{f,i}(k)), complex128, for kx and ky (1/Angstrom) that broadcast against each other"""
        kx, ky = np.asarray(kx, dtype=np.float64), np.asarray(ky, dtype=np.float64)
        p = self.polar(f, i)
        names = ("C10", "C12", "C21", "C23", "C30", "C32", "C34", "C41", "C43", "C45", "C50", "C52", "C54", "C56")
        kw = {}
        for (c, phi), name in zip(p, names):
            kw[name] = c
            if name[2] != "0":
                kw["phi" + name[1:]] = phi
        H = np.exp(-1j * Aberrations(**kw).chi(kx, ky, wavelength))
        if self.aperture_mrad is not None:
            H = np.where(np.sqrt(kx * kx + ky * ky) < self.aperture_k(wavelength), H, 0.0)
        return H
