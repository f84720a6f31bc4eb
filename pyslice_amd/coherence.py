"""Partial coherence of the STEM probe: MultisliceCalculator(coherence=Coherence(...)).

A real probe is an incoherent ensemble.  The energy spread of the gun smears the defocus through the chromatic aberration
(temporal coherence: a Gaussian of rms width Delta, 30-80 Angstrom on an uncorrected instrument), and the demagnified source has a
finite size at the specimen (spatial coherence: an isotropic Gaussian of rms width sigma_s per axis, 0.3-0.8 Angstrom).  Both
average INTENSITIES over the ensemble, so every signal of scan position q is

    S[q] = sum_g w_g S(xy[q] + d_g, C10 + delta_g),        sum_g w_g = 1

over G member probes: Gauss-Hermite nodes of the focal distribution, delta_f = sqrt(2) Delta x_f with weights omega_f / sqrt(pi)
from numpy.polynomial.hermite.hermgauss(F) -- the rule of imaging.Imaging.focal_spread -- times the S x S tensor rule of the source,
d = sqrt(2) sigma_s (x_ix, x_iy).  G = F S^2 members in the fixed order g = (f S + ix) S + iy, the weight of a member the product of
its node weights.

The members ride through the slice loop as ordinary probes of the batch (wave q G + g); msl_diffract_members / msl_dose_add_members
fold the G patterns of a position into one on the device (csrc/ensemble.h), before the Poisson draw of a dose run; the small
detector and polar signals are folded on the host in float64, in member order.  The price is G slice loops per position; the
potentials are built as often as without.  For a source size alone, on a regular raster, without a dose, `blur_scan` below is the
cheap route: the convolution of the finished scan with the source.

Sign convention: delta_g is added to C10 in this project's sense, C10 = +dz being the reference's Probe.defocus(dz).
Not in the reference, whose probe is perfectly coherent.
"""
from __future__ import annotations

import math
from dataclasses import dataclass

import numpy as np

MEMBERS_MAX = 128           # include/mslice.h: MSL_MEMBERS_MAX
ELECTRON_REST_EV = 511e3    # E0 of chromatic_focal_spread


def _number(name, v, who="Coherence"):
    if isinstance(v, (bool, np.bool_)):
        raise ValueError(f"{who}: {name} must be a number, got {v!r}")
    try:
        v = float(v)
    except (TypeError, ValueError):
        raise ValueError(f"{who}: {name} must be a number, got {v!r}") from None
    if not math.isfinite(v):
        raise ValueError(f"{who}: {name} must be finite, got {v}")
    if v < 0:
        raise ValueError(f"{who}: {name} must not be negative, got {v}")
    return v


def _points(name, n, width_name, width):
    if isinstance(n, (bool, np.bool_)) or not isinstance(n, (int, np.integer)) or int(n) < 1 or int(n) % 2 == 0:
        raise ValueError(f"Coherence: {name} must be an odd integer >= 1, got {n!r}")
    if int(n) > 1 and width == 0:
        raise ValueError(f"Coherence: {name} > 1 needs {width_name} > 0")
    return int(n)


def _hermite(n, width):
    """(nodes, weights) of the n-point Gauss-Hermite rule of a Gaussian of standard deviation `width`; (0, 1) at one point"""
    if n == 1 or width == 0:
        return np.array([0.0]), np.array([1.0])
    x, w = np.polynomial.hermite.hermgauss(n)
    return math.sqrt(2.0) * width * x, w / math.sqrt(math.pi)


@dataclass(frozen=True)
class Coherence:
    """focal_spread: rms defocus width Delta (Angstrom); focal_points: odd number F of Gauss-Hermite nodes (F > 1 needs
    focal_spread > 0); source_size: rms width sigma_s (Angstrom) per axis of the Gaussian source image at the specimen;
    source_points: odd number S of nodes per axis, the S x S tensor rule (S > 1 needs source_size > 0).  F S^2 <= 128.  A
    non-finite or negative width, an even or non-positive point count and more than 128 members raise ValueError.  Coherence() is
    off: one member of weight 1 at offset 0."""
    focal_spread: float = 0.0
    focal_points: int = 1
    source_size: float = 0.0
    source_points: int = 1

    def __post_init__(self):
        spread = _number("focal_spread", self.focal_spread)
        size = _number("source_size", self.source_size)
        object.__setattr__(self, "focal_spread", spread)
        object.__setattr__(self, "source_size", size)
        object.__setattr__(self, "focal_points", _points("focal_points", self.focal_points, "focal_spread", spread))
        object.__setattr__(self, "source_points", _points("source_points", self.source_points, "source_size", size))
        if self.n_members > MEMBERS_MAX:
            raise ValueError(f"Coherence: {self.focal_points} x {self.source_points}^2 = {self.n_members} members, at most {MEMBERS_MAX}")

    @property
    def n_members(self):
        """G = F S^2"""
        return self.focal_points * self.source_points ** 2

    @property
    def is_off(self):
        """one member: the coherent probe"""
        return self.n_members == 1

    def focal_nodes(self):
        """(delta_f, w_f): the defocus offsets (Angstrom) and weights (sum 1) of the focal average, as Imaging.nodes()"""
        return _hermite(self.focal_points, self.focal_spread)

    def source_nodes(self):
        """(d_i, w_i): the offsets (Angstrom) and weights (sum 1) of the source average along one axis"""
        return _hermite(self.source_points, self.source_size)

    def members(self):
        """(offsets (G, 2), defocus (G,), weights (G,)) float64 in the order g = (f S + ix) S + iy"""
        df, wf = self.focal_nodes()
        ds, ws = self.source_nodes()
        F, S = len(df), len(ds)
        offsets = np.zeros((F, S, S, 2), dtype=np.float64)
        offsets[..., 0] = ds[None, :, None]
        offsets[..., 1] = ds[None, None, :]
        defocus = np.broadcast_to(df[:, None, None], (F, S, S))
        weights = wf[:, None, None] * (ws[None, :, None] * ws[None, None, :])
        return (offsets.reshape(-1, 2), np.ascontiguousarray(defocus, dtype=np.float64).reshape(-1),
                np.ascontiguousarray(weights, dtype=np.float64).reshape(-1))


def chromatic_focal_spread(Cc, energy_spread_eV, voltage_eV):
    """rms defocus width (the unit of Cc) of an rms energy spread: Cc dE/E (1 + E/E0) / (1 + E/2E0), E0 = 511 keV"""
    E = float(voltage_eV)
    return float(Cc) * float(energy_spread_eV) / E * (1.0 + E / ELECTRON_REST_EV) / (1.0 + E / (2.0 * ELECTRON_REST_EV))


def fwhm_to_sigma(fwhm):
    """standard deviation of a Gaussian of the given full width at half maximum"""
    return float(fwhm) / (2.0 * math.sqrt(2.0 * math.log(2.0)))


def fold_members(values, weights):
    """(Q G, ...) per-wave values -> (Q, ...): sum_g w_g values[q G + g], float64, added in member order"""
    v = np.asarray(values, dtype=np.float64)
    w = np.asarray(weights, dtype=np.float64).reshape(-1)
    G = len(w)
    if v.shape[0] % G:
        raise ValueError(f"fold_members: {v.shape[0]} waves are no multiple of {G} members")
    v = v.reshape((v.shape[0] // G, G) + v.shape[1:])
    out = np.zeros((v.shape[0],) + v.shape[2:], dtype=np.float64)
    for g in range(G):
        out += w[g] * v[:, g]
    return out


def blur_scan(values, step_xy, sigma, periodic=True):
    """`values` (nx_scan, ny_scan, ...) of a regular raster with steps step_xy = (sx, sy) in Angstrom, convolved along its two
    leading axes with the Gaussian source of rms width sigma per axis.  periodic=True: the scan covers a periodic cell -- the
    product with exp(-2 pi^2 sigma^2 q^2) in the scan's Fourier space.  periodic=False: the same after padding each side by
    ceil(4 sigma / step) points of edge-replicated values, the pad cut off again.  sigma = 0 returns a float64 copy."""
    v = np.array(values, dtype=np.float64)
    sigma = _number("sigma", sigma, "blur_scan")
    if v.ndim < 2:
        raise ValueError(f"blur_scan: values must have two leading scan axes, got shape {v.shape}")
    sx, sy = float(step_xy[0]), float(step_xy[1])
    if not (sx > 0 and sy > 0 and math.isfinite(sx) and math.isfinite(sy)):
        raise ValueError(f"blur_scan: steps must be positive, got {step_xy!r}")
    if sigma == 0:
        return v
    pad = (0, 0) if periodic else (int(math.ceil(4.0 * sigma / sx)), int(math.ceil(4.0 * sigma / sy)))
    if not periodic:
        v = np.pad(v, [(pad[0], pad[0]), (pad[1], pad[1])] + [(0, 0)] * (v.ndim - 2), mode="edge")
    qx = np.fft.fftfreq(v.shape[0], d=sx)
    qy = np.fft.fftfreq(v.shape[1], d=sy)
    damp = np.exp(-2.0 * math.pi ** 2 * sigma ** 2 * (qx[:, None] ** 2 + qy[None, :] ** 2))
    damp = damp.reshape(damp.shape + (1,) * (v.ndim - 2))
    out = np.fft.ifft2(np.fft.fft2(v, axes=(0, 1)) * damp, axes=(0, 1)).real
    if not periodic:
        out = out[pad[0]:out.shape[0] - pad[0], pad[1]:out.shape[1] - pad[1]]
    return np.ascontiguousarray(out)


def blur_positions(values, probe_positions, sigma, periodic=True):
    """blur_scan of a result whose leading axis runs over `probe_positions` (P, ...): the positions must form a full regular raster
    (the test of Dose(per_area=...)), in any order; ValueError otherwise"""
    from .dose import raster_steps
    from .stem_data import scan_axes
    pp = np.asarray(probe_positions, dtype=np.float64).reshape(-1, 2)
    v = np.asarray(values, dtype=np.float64)
    if v.shape[0] != len(pp):
        raise ValueError(f"source_blurred: {v.shape[0]} rows for {len(pp)} probe positions")
    steps = raster_steps(pp, "source_blurred")
    xs, ys = scan_axes(pp)
    ix = np.abs(pp[:, 0][:, None] - np.asarray(xs)[None, :]).argmin(axis=1)
    iy = np.abs(pp[:, 1][:, None] - np.asarray(ys)[None, :]).argmin(axis=1)
    grid = np.zeros((len(xs), len(ys)) + v.shape[1:], dtype=np.float64)
    grid[ix, iy] = v
    out = blur_scan(grid, steps, sigma, periodic=periodic)
    return np.ascontiguousarray(out[ix, iy])
