"""Aberration function of the probe-forming lens (not in the reference, whose only aberration is Probe.defocus()).

    psi0[p] = ifft2( A(k) * ramp_p(k) * exp(-i chi(k)) )

    chi(k) = (2 pi / lambda) * sum_nm  C_nm / (n + 1) * alpha^(n+1) * cos(m (phi - phi_nm)),
    alpha = lambda |k|,  phi = atan2(ky, kx)

with the fourteen terms through fifth order in the order of TERMS (msl_set_aberrations takes them in this order).  Magnitudes are
in Angstrom, angles in radians; terms with m = 0 have no angle.

Sign: C10 = +dz is the reference's Probe.defocus(dz) for dz > 0, exp(-i pi lambda dz k^2): a positive defocus puts the beam waist
above the sample.  This is the OPPOSITE of abTEM, where defocus = -C10.  A negative C10 is a true negative defocus, the
complex-conjugate phase -- unlike Probe.defocus(), where both signs defocus by +|dz| (quirk Q19, left as it is).

The device evaluates chi in the analytic reciprocal-space probe kernel (probe_kspace_aberr_kernel); `Aberrations.chi` below is
the float64 NumPy statement of the same formula, which the tests compare against.
"""
from __future__ import annotations

import math
from dataclasses import InitVar, dataclass, fields
from typing import Optional

import numpy as np

# (name, n, m) in the order of msl_set_aberrations
TERMS = (("C10", 1, 0), ("C12", 1, 2), ("C21", 2, 1), ("C23", 2, 3), ("C30", 3, 0), ("C32", 3, 2), ("C34", 3, 4),
         ("C41", 4, 1), ("C43", 4, 3), ("C45", 4, 5), ("C50", 5, 0), ("C52", 5, 2), ("C54", 5, 4), ("C56", 5, 6))
# keyword alias -> field
ALIASES = {"defocus": "C10", "astigmatism": "C12", "astigmatism_angle": "phi12", "coma": "C21", "coma_angle": "phi21",
           "Cs": "C30", "C5": "C50"}


@dataclass(frozen=True)
class Aberrations:
    """The fourteen coefficients C_nm (Angstrom) and the angles phi_nm (radians) of the terms with m > 0.

    Keyword aliases: defocus (C10), astigmatism / astigmatism_angle (C12 / phi12), coma / coma_angle (C21 / phi21), Cs (C30),
    C5 (C50).  An alias given together with a non-zero value of its field raises ValueError; so does any non-finite value.
    defocus = +dz is Probe.defocus(dz) of the reference for dz > 0 -- the opposite sign of abTEM's defocus = -C10.
    """
    C10: float = 0.0
    C12: float = 0.0
    phi12: float = 0.0
    C21: float = 0.0
    phi21: float = 0.0
    C23: float = 0.0
    phi23: float = 0.0
    C30: float = 0.0
    C32: float = 0.0
    phi32: float = 0.0
    C34: float = 0.0
    phi34: float = 0.0
    C41: float = 0.0
    phi41: float = 0.0
    C43: float = 0.0
    phi43: float = 0.0
    C45: float = 0.0
    phi45: float = 0.0
    C50: float = 0.0
    C52: float = 0.0
    phi52: float = 0.0
    C54: float = 0.0
    phi54: float = 0.0
    C56: float = 0.0
    phi56: float = 0.0
    defocus: InitVar[Optional[float]] = None
    astigmatism: InitVar[Optional[float]] = None
    astigmatism_angle: InitVar[Optional[float]] = None
    coma: InitVar[Optional[float]] = None
    coma_angle: InitVar[Optional[float]] = None
    Cs: InitVar[Optional[float]] = None
    C5: InitVar[Optional[float]] = None

    def __post_init__(self, defocus, astigmatism, astigmatism_angle, coma, coma_angle, Cs, C5):
        given = dict(defocus=defocus, astigmatism=astigmatism, astigmatism_angle=astigmatism_angle, coma=coma,
                     coma_angle=coma_angle, Cs=Cs, C5=C5)
        for alias, value in given.items():
            if value is None:
                continue
            name = ALIASES[alias]
            if getattr(self, name) != 0:
                raise ValueError(f"{alias} and {name} name the same coefficient: give one of them")
            object.__setattr__(self, name, value)
        for f in fields(self):
            try:
                v = float(getattr(self, f.name))
            except (TypeError, ValueError):
                raise ValueError(f"{f.name} must be a number, got {getattr(self, f.name)!r}") from None
            if not math.isfinite(v):
                raise ValueError(f"{f.name} must be finite, got {v}")
            object.__setattr__(self, f.name, v)

    @classmethod
    def from_dict(cls, d):
        """from a mapping of field names and / or aliases; an unknown key raises ValueError"""
        known = {f.name for f in fields(cls)} | set(ALIASES)
        for k in d:
            if k not in known:
                raise ValueError(f"unknown aberration {k!r} (known: {sorted(known)})")
        return cls(**dict(d))

    def as_polar(self):
        """(14, 2) float64: (magnitude, angle) per term in the order of TERMS; the angle of an m = 0 term is 0"""
        return np.array([[getattr(self, name), getattr(self, "phi" + name[1:]) if m else 0.0] for name, n, m in TERMS],
                        dtype=np.float64)

    @property
    def is_zero(self):
        """every magnitude is zero: the probe is the un-aberrated one whatever the angles say"""
        return not np.any(self.as_polar()[:, 0])

    def chi(self, kx, ky, wavelength):
        """chi(k) in radians, float64, for kx and ky (1/Angstrom) that broadcast against each other"""
        kx, ky = np.asarray(kx, dtype=np.float64), np.asarray(ky, dtype=np.float64)
        alpha = wavelength * np.hypot(kx, ky)
        phi = np.arctan2(ky, kx)
        total = np.zeros(np.broadcast(kx, ky).shape, dtype=np.float64)
        for (name, n, m), (c, phi0) in zip(TERMS, self.as_polar()):
            if c != 0:
                total = total + c / (n + 1) * alpha ** (n + 1) * np.cos(m * (phi - phi0))
        return 2 * np.pi / wavelength * total


def scherzer_defocus(Cs, eV):
    """-sqrt(1.5 Cs lambda) in Angstrom (Cs in Angstrom): the C10 that balances a positive Cs in this module's sign convention"""
    from .multislice import wavelength
    return -math.sqrt(1.5 * Cs * wavelength(eV))
