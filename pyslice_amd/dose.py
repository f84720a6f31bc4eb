"""Finite dose: Poisson-counted signals at a stated number of electrons, reproducible from a seed.

Every scan mode returns noise-free expectation values.  A detector records electron counts: a pixel whose expectation is `lam`
electrons records a Poisson variate of mean `lam`.  This file is the definition of that draw, in NumPy, float64 and integers only;
the device makes the same draws itself (csrc/dose.h: dose_counts_kernel behind msl_dose_counts), where the patterns already are, so
a 4D-STEM scan downloads 4 bytes per detector pixel instead of 8 and the noise is a pure function of (seed, probe, pixel).

Random stream.  The draws of pixel i (row-major index in the (mx, my) pattern) of probe p (the global probe index of the scan, not
the index inside a probe batch: the counts do not depend on probe_batch) come from Philox-4x32-10 (thermal.philox4x32_10):

    key      (seed & 0xffffffff, seed >> 32)
    counter  (i, p, attempt, 0)                 attempt = 0, 1, ... : one block x0..x3 per attempt
    U(hi, lo) = (((hi >> 6) << 26 | (lo >> 6)) + 0.5) * 2^-52       an odd multiple of 2^-53 in (0, 1), exact in float64
    u = U(x0, x1)      v = U(x2, x3)

lam == 0 gives 0 without drawing.

lam < 10: inversion by sequential search on the u of attempt 0,
    p = exp(-lam); s = p; k = 0;  while u > s and k < K_LIMIT (96): k += 1; p *= lam / k; s += p
(one exp; P(k > 96) < 1e-50 at lam < 10, so the bound is reached only where the rounded sum stays below u, about 1e-15 per draw).

lam >= 10: Hoermann's transformed rejection PTRS ("The transformed rejection method for generating Poisson random variables",
Insurance: Mathematics and Economics 12 (1993)), the algorithm of NumPy's generator, one block (u, v) per attempt:
    slam = sqrt(lam); loglam = log(lam); b = 0.931 + 2.53 slam; a = -0.059 + 0.02483 b
    invalpha = 1.1239 + 1.1328 / (b - 3.4); vr = 0.9277 - 3.6224 / (b - 2)
    U = u - 0.5; us = 0.5 - |U|; k = floor((2 a / us + b) U + lam + 0.43)
    us >= 0.07 and v <= vr:                                                        accept k
    k < 0 or (us < 0.013 and v > us):                                              next attempt
    log(v) + log(invalpha) - log(a / us^2 + b) <= -lam + k loglam - lgamma(k + 1): accept k
at most ATTEMPTS (64), then rint(lam): an attempt accepts with probability above 0.85, so that is not reached in practice.
Every product and sum rounds on its own (no fused multiply-add), on the host and on the device.  Counts saturate at 2^32 - 1.

The device may differ from this file only where its exp / log / lgamma differ from the host's in the last place AND that flips
one of the comparisons above: about 1e-13 per pixel.

The detector's response to these counts -- point spread, gain, offset, readout noise, uint16 frames -- is camera.py.
Not built: dose on the device for polar and STEM-detector signals (their arrays are small: poisson_signals below, on the host), dose
under PRISM, thickness series and precession.
"""
from __future__ import annotations

import math

import numpy as np

from .thermal import _u64, philox4x32_10

K_LIMIT = 96            # inversion: the largest count of lam < 10
ATTEMPTS = 64           # PTRS: attempts before rint(lam)
PTRS_FROM = 10.0        # lam >= 10: PTRS
COUNT_MAX = 2 ** 32 - 1

_lgamma = np.frompyfunc(math.lgamma, 1, 1)


def _uniform53(hi, lo):
    """U(hi, lo) of two uint32 words: an odd multiple of 2^-53 in (0, 1)"""
    m = ((hi.astype(np.uint64) >> np.uint64(6)) << np.uint64(26)) | (lo.astype(np.uint64) >> np.uint64(6))
    return (m.astype(np.float64) + 0.5) * 2.0 ** -52


def _block(pixel, probe, attempt, key):
    """(u, v) of attempt `attempt` for the pixels / probes given (uint32 arrays of one shape)"""
    ctr = np.zeros(pixel.shape + (4,), dtype=np.uint32)
    ctr[..., 0], ctr[..., 1], ctr[..., 2] = pixel, probe, attempt
    x = philox4x32_10(ctr, key)
    return _uniform53(x[..., 0], x[..., 1]), _uniform53(x[..., 2], x[..., 3])


def _saturate(k):
    return np.where(k >= float(COUNT_MAX), COUNT_MAX, np.where(k > 0, k, 0.0)).astype(np.uint64).astype(np.uint32)


def _invert(lam, u):
    p = np.exp(-lam)
    s = p.copy()
    k = np.zeros(lam.shape, dtype=np.float64)
    for _ in range(K_LIMIT):
        go = u > s
        if not go.any():
            break
        k = np.where(go, k + 1.0, k)
        kk = np.where(go, k, 1.0)
        p = np.where(go, p * (lam / kk), p)
        s = np.where(go, s + p, s)
    return k


def _ptrs(lam, pixel, probe, key):
    out = np.rint(lam)                                      # what is left after ATTEMPTS rejections
    slam, loglam = np.sqrt(lam), np.log(lam)
    b = 0.931 + 2.53 * slam
    a = -0.059 + 0.02483 * b
    invalpha = 1.1239 + 1.1328 / (b - 3.4)
    vr = 0.9277 - 3.6224 / (b - 2.0)
    live = np.arange(lam.size)
    with np.errstate(over="ignore", invalid="ignore"):
        for attempt in range(ATTEMPTS):
            if live.size == 0:
                break
            u, v = _block(pixel[live], probe[live], np.uint32(attempt), key)
            l, al, bl = lam[live], a[live], b[live]
            U = u - 0.5
            us = 0.5 - np.abs(U)
            k = np.floor((2.0 * al / us + bl) * U + l + 0.43)
            fast = (us >= 0.07) & (v <= vr[live])
            skip = ~fast & ((k < 0) | ((us < 0.013) & (v > us)))
            slow = ~fast & ~skip
            acc = fast.copy()
            if slow.any():
                j = np.flatnonzero(slow)
                lhs = np.log(v[j]) + np.log(invalpha[live][j]) - np.log(al[j] / (us[j] * us[j]) + bl[j])
                rhs = -l[j] + k[j] * loglam[live][j] - _lgamma(k[j] + 1.0).astype(np.float64)
                acc[j] = lhs <= rhs
            out[live[acc]] = k[acc]
            live = live[~acc]
    return out


def poisson_counts(lam, seed, probe_index):
    """The Poisson draws of the module's definition -> uint32 of lam's shape.  probe_index an integer: lam is the pattern of that
    probe (any shape; the pixel index is the row-major index).  probe_index a sequence of P integers: lam is (P, ...) and lam[j] is
    the pattern of probe probe_index[j].  ValueError for a negative or non-finite lam."""
    lam = np.asarray(lam, dtype=np.float64)
    seed = _u64("seed", seed)
    if np.ndim(probe_index) == 0:
        probes = np.asarray([probe_index])
        pats = lam.reshape(1, -1)
    else:
        probes = np.asarray(probe_index).reshape(-1)
        if lam.ndim < 1 or lam.shape[0] != probes.size:
            raise ValueError(f"poisson_counts: lam of shape {lam.shape} for {probes.size} probes")
        pats = lam.reshape(probes.size, -1)
    if probes.size and (probes.dtype.kind not in "iu" or probes.min() < 0 or probes.max() > COUNT_MAX):
        raise ValueError("poisson_counts: probe indices must be integers in [0, 2^32)")
    if pats.shape[1] > COUNT_MAX:
        raise ValueError("poisson_counts: more than 2^32 - 1 pixels per pattern")
    if not np.all(np.isfinite(pats)) or np.any(pats < 0):
        raise ValueError("poisson_counts: lam must be finite and >= 0")
    key = (seed & 0xFFFFFFFF, seed >> 32)
    flat = pats.reshape(-1)
    pixel = np.tile(np.arange(pats.shape[1], dtype=np.uint32), probes.size)
    probe = np.repeat(probes.astype(np.uint32), pats.shape[1])
    k = np.zeros(flat.shape, dtype=np.float64)
    small = np.flatnonzero((flat > 0) & (flat < PTRS_FROM))
    if small.size:
        u, _ = _block(pixel[small], probe[small], np.uint32(0), key)
        k[small] = _invert(flat[small], u)
    large = np.flatnonzero(flat >= PTRS_FROM)
    if large.size:
        k[large] = _ptrs(flat[large], pixel[large], probe[large], key)
    return _saturate(k).reshape(lam.shape)


def incident_intensity(nx, ny, dx, dy, mrad, wavelength):
    """I_incident: the sum of |Psi|^2 over the whole unnormalised spectrum of the incident probe -- the number of grid pixels inside
    the aperture (the probe's spectrum is a unit phase on each, prism.beams' rule), (nx ny)^2 for a plane wave (mrad = 0)"""
    if not mrad > 0:
        return float(nx * ny) ** 2
    from .prism import beams
    return float(len(beams(int(nx), int(ny), float(dx), float(dy), float(mrad), float(wavelength))))


def raster_steps(probe_positions, who, hint=""):
    """(step_x, step_y) of a scan that is a full regular raster of its coordinates (stem_data.scan_axes).  ValueError, opened with
    `who` and closed with `hint`, for anything else (missing raster points, uneven steps, a single row or column)."""
    from .stem_data import scan_axes
    pp = np.asarray(probe_positions, dtype=np.float64).reshape(-1, 2)
    xs, ys = scan_axes(pp)
    steps = []
    for name, ax in (("x", xs), ("y", ys)):
        d = np.diff(ax)
        if d.size < 1 or not np.allclose(d, d[0], rtol=1e-6, atol=1e-9):
            raise ValueError(f"{who}: the scan is not a regular raster along {name}{hint}")
        steps.append(float(d[0]))
    if len(xs) * len(ys) != len(pp) or len({(x, y) for x, y in pp}) != len(pp):
        raise ValueError(f"{who}: the probe positions are not a full raster of their coordinates{hint}")
    return steps[0], steps[1]


def scan_step_area(probe_positions):
    """the area (Angstrom^2) one probe position stands for in a regular raster scan: the product of the steps of
    stem_data.scan_axes.  ValueError for anything else (missing raster points, uneven steps, a single row or column)."""
    sx, sy = raster_steps(probe_positions, "Dose(per_area=...)", " (give electrons_per_probe)")
    return sx * sy


def _dose_number(name, v):
    if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, float, np.integer, np.floating)) or not np.isfinite(v) or v < 0:
        raise ValueError(f"Dose: {name} must be a finite number >= 0, got {v!r}")
    return float(v)


class Dose:
    """The request: electrons_per_probe, or per_area in electrons / Angstrom^2 (times the step area of the regular scan) -- exactly
    one of the two; seed, a non-negative 64-bit integer, is the key of the draws; keep_intensity=True also keeps the float64
    noise-free result next to the counts."""

    def __init__(self, electrons_per_probe=None, per_area=None, seed=0, keep_intensity=False):
        if (electrons_per_probe is None) == (per_area is None):
            raise ValueError("Dose: give exactly one of electrons_per_probe and per_area")
        self.electrons_per_probe = None if electrons_per_probe is None else _dose_number("electrons_per_probe", electrons_per_probe)
        self.per_area = None if per_area is None else _dose_number("per_area", per_area)
        self.seed = _u64("seed", seed)
        if not isinstance(keep_intensity, (bool, np.bool_)):
            raise ValueError(f"Dose: keep_intensity must be True or False, got {keep_intensity!r}")
        self.keep_intensity = bool(keep_intensity)

    def electrons(self, probe_positions):
        """electrons per probe position of this dose on the scan `probe_positions`"""
        if self.electrons_per_probe is not None:
            return self.electrons_per_probe
        return self.per_area * scan_step_area(probe_positions)

    def __repr__(self):
        what = f"electrons_per_probe={self.electrons_per_probe:g}" if self.per_area is None else f"per_area={self.per_area:g}"
        return f"Dose({what}, seed={self.seed}" + (", keep_intensity=True)" if self.keep_intensity else ")")


def poisson_signals(signals, electrons_per_probe, incident, seed):
    """Host-side counts of small per-probe signals (STEMData.poisson, PolarData.poisson): signals (P, ...) in the units of the
    unnormalised spectra, lam = signals * (electrons_per_probe / incident), probe p keyed by its row, the pixel index the row-major
    index of the rest -> uint32 of the same shape"""
    n_e = _dose_number("dose", electrons_per_probe)
    s = np.asarray(signals, dtype=np.float64)
    return poisson_counts(s * (n_e / float(incident)), seed, np.arange(s.shape[0], dtype=np.int64))


def probe_incident(probe):
    """incident_intensity of a multislice.Probe (the analytic probe of a run); a custom array is summed as it is"""
    if probe is None:
        raise ValueError("poisson(): the result carries no probe, so the incident intensity is not known")
    if getattr(probe, "_custom", False):
        a = probe.array
        a = a.detach().cpu().numpy() if hasattr(a, "detach") else np.asarray(a)
        return float((np.abs(np.fft.fft2(a.reshape((-1,) + a.shape[-2:])[0])) ** 2).sum())
    return incident_intensity(probe._nx, probe._ny, probe._dx, probe._dy, probe.mrad, probe.wavelength)
