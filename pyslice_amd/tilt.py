"""Specimen tilt and precession (not in the reference, whose beam always travels along the slice normal).

Tilt (theta_x, theta_y) is the inclination of the beam to the slice normal, small-angle: the specimen is sheared, not rotated.
Free propagation through one slice of thickness dz moves the wave by (+dz tan theta_x, +dz tan theta_y), cyclically (the cell is
periodic).  With the transform convention Psi(k) = sum_r psi(r) exp(-2 pi i k.r) the propagator of one slice is

    P_tilt(kx, ky) = exp(-i pi lambda dz kx^2) exp(-2 pi i dz kx tan theta_x)  x  exp(-i pi lambda dz ky^2) exp(-2 pi i dz ky tan theta_y)

-- still separable, one linear phase per axis.  The pattern stays centred on the optic axis: the beam is along z and the specimen
is sheared, so nothing needs de-rocking.  The device writes the tables of P_tilt itself (msl_set_tilt, csrc/propagator.h);
`tilted_propagator` and `propagate_tilted` below are the float64 NumPy statement of the same formula, which the tests compare
against.  A precession run is a loop over the tilts of a cone (Precession), averaged on the host.
"""
from __future__ import annotations

import math

import numpy as np

MAX_MRAD = 200.0        # the small-angle (shear) form is not meant beyond this


class Tilt:
    """MultisliceCalculator(tilt=Tilt(x_mrad, y_mrad)) / Propagate(..., tilt=): the inclination of the beam along x and y in mrad.
    ValueError for a non-finite angle or |angle| > 200 mrad on either axis.  Tilt() is no tilt: every output is bit for bit that of
    a run without the argument."""

    __slots__ = ("x_mrad", "y_mrad")

    def __init__(self, x_mrad=0.0, y_mrad=0.0):
        for name, v in (("x_mrad", x_mrad), ("y_mrad", y_mrad)):
            if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, float, np.integer, np.floating)) or not math.isfinite(v):
                raise ValueError(f"Tilt: {name} must be a finite angle in mrad, got {v!r}")
            if abs(v) > MAX_MRAD:
                raise ValueError(f"Tilt: {name} = {v:g} mrad is beyond the small-angle form (|angle| <= {MAX_MRAD:g} mrad)")
        object.__setattr__(self, "x_mrad", float(x_mrad))
        object.__setattr__(self, "y_mrad", float(y_mrad))

    def __setattr__(self, name, value):
        raise AttributeError("Tilt is immutable")

    @property
    def is_zero(self):
        return self.x_mrad == 0.0 and self.y_mrad == 0.0

    @property
    def tangents(self):
        """(tan theta_x, tan theta_y): what msl_set_tilt takes"""
        return math.tan(self.x_mrad * 1e-3), math.tan(self.y_mrad * 1e-3)

    @classmethod
    def from_shift(cls, shift_x, shift_y, dz):
        """the tilt that moves the wave by (shift_x, shift_y) Angstrom per slice of thickness dz"""
        return cls(math.atan2(shift_x, dz) * 1e3, math.atan2(shift_y, dz) * 1e3)

    def __eq__(self, other):
        return isinstance(other, Tilt) and (self.x_mrad, self.y_mrad) == (other.x_mrad, other.y_mrad)

    def __hash__(self):
        return hash((self.x_mrad, self.y_mrad))

    def __repr__(self):
        return f"Tilt(x_mrad={self.x_mrad:g}, y_mrad={self.y_mrad:g})"


def as_tilt(value, what="tilt"):
    """None or a Tilt -> a Tilt"""
    if value is None:
        return Tilt()
    if not isinstance(value, Tilt):
        raise ValueError(f"{what}: expected a Tilt object, got {value!r}")
    return value


class Precession:
    """MultisliceCalculator(precession=Precession(angle_mrad, n_azimuth, phase0, centre)): n_azimuth tilts on a cone of half-angle
    angle_mrad around `centre`, tilt i at azimuth phase0 + 2 pi i / n_azimuth (radians):
        Tilt(centre.x_mrad + angle_mrad cos(azimuth), centre.y_mrad + angle_mrad sin(azimuth)).
    run_diffraction(), run_polar() and run_detectors() return the mean of the single-tilt results over the cone.  ValueError for
    n_azimuth < 1, a negative or non-finite angle, or a tilt of the cone beyond 200 mrad."""

    def __init__(self, angle_mrad, n_azimuth, phase0=0.0, centre=None):
        if isinstance(n_azimuth, (bool, np.bool_)) or not isinstance(n_azimuth, (int, np.integer)) or int(n_azimuth) < 1:
            raise ValueError(f"Precession: n_azimuth must be a positive integer, got {n_azimuth!r}")
        if not (isinstance(angle_mrad, (int, float, np.integer, np.floating)) and math.isfinite(angle_mrad) and angle_mrad >= 0):
            raise ValueError(f"Precession: angle_mrad must be a finite angle >= 0, got {angle_mrad!r}")
        if not (isinstance(phase0, (int, float, np.integer, np.floating)) and math.isfinite(phase0)):
            raise ValueError(f"Precession: phase0 must be a finite azimuth in radians, got {phase0!r}")
        self.angle_mrad, self.n_azimuth, self.phase0 = float(angle_mrad), int(n_azimuth), float(phase0)
        self.centre = as_tilt(centre, "Precession: centre")
        self._tilts = []
        for i in range(self.n_azimuth):
            az = self.phase0 + 2.0 * math.pi * i / self.n_azimuth
            self._tilts.append(Tilt(self.centre.x_mrad + self.angle_mrad * math.cos(az),
                                    self.centre.y_mrad + self.angle_mrad * math.sin(az)))

    def tilts(self):
        """the n_azimuth Tilt objects, in the order the runs are made and averaged"""
        return list(self._tilts)

    def __iter__(self):
        return iter(self._tilts)

    def __len__(self):
        return self.n_azimuth

    def __repr__(self):
        return f"Precession(angle_mrad={self.angle_mrad:g}, n_azimuth={self.n_azimuth}, phase0={self.phase0:g}, centre={self.centre!r})"


def tilted_propagator(nx, ny, dx, dy, wavelength, dz, tilt=None):
    """(nx, ny) complex128: P_tilt on the unshifted grid (numpy's fftfreq order).  Tilt() gives exp(-i pi lambda dz (kx^2 + ky^2)),
    the reference's propagator, exactly."""
    tilt = as_tilt(tilt)
    kxs = np.fft.fftfreq(nx, d=dx)
    kys = np.fft.fftfreq(ny, d=dy)
    prop = np.exp(-1j * np.pi * wavelength * dz * (kxs[:, None] ** 2 + kys[None, :] ** 2))
    if tilt.is_zero:
        return prop
    tx, ty = tilt.tangents
    turns = dz * (kxs[:, None] * tx + kys[None, :] * ty)
    return prop * np.exp(-2j * np.pi * (turns - np.rint(turns)))


def propagate_tilted(psi0, transmission, dx, dy, wavelength, dz, tilt=None, layers=None):
    """The slice loop in float64: psi0 (P, nx, ny) or (nx, ny) incident waves, transmission (nz, nx, ny) complex (slice-major,
    exp(i sigma V) of every slice; all ones is vacuum) -> exit waves (P, nx, ny) complex128 after nz transmissions and nz - 1
    propagations with P_tilt.  layers = slice indices k: also returns {k: the waves after the transmission of slice k}, the
    definition of MultisliceCalculator(layers=...) -> (exit, taps)."""
    psi = np.array(psi0, dtype=np.complex128)
    if psi.ndim == 2:
        psi = psi[None]
    t = np.asarray(transmission)
    if t.ndim != 3 or t.shape[1:] != psi.shape[1:]:
        raise ValueError(f"propagate_tilted: transmission {t.shape} does not match the waves {psi.shape}: expected (nz, nx, ny)")
    nz, nx, ny = t.shape
    prop = tilted_propagator(nx, ny, dx, dy, wavelength, dz, tilt)
    taps = {}
    for z in range(nz):
        psi = t[z][None] * psi
        if layers is not None and z in layers:
            taps[int(z)] = psi.copy()
        if z < nz - 1:
            psi = np.fft.ifft2(prop[None] * np.fft.fft2(psi, axes=(-2, -1)), axes=(-2, -1))
    return psi if layers is None else (psi, taps)
