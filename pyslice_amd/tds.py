"""TDS detector signal of the absorptive potential: HAADF from ONE pass.

The absorptive potential (absorptive.py) takes the thermal diffuse scattering out of the elastic wave and drops it.  High-angle
annular dark field is almost entirely that TDS.  This file is the float64 definition of where it lands, in the local approximation
on top of the second-cumulant model: the intensity that slice s removes at pixel r, |psi_s(r)|^2 (1 - |t_s(r)|^2), is split over
the detectors by the covariance of V integrated against each detector's real-space response.  With M the detector's membership on
the fftfreq grid (Detector.member(fftfreq(nx, dx), fftfreq(ny, dy), wavelength): unshifted, no window), per species and in the
notation of absorptive.py

    V1M    = real(ifft2(M f))   / (dx^2 dy^2)        Vbar1M = real(ifft2(M f D)) / (dx^2 dy^2)
    Om1det = 1/2 (real(ifft2(D fft2(V1 V1M))) - Vbar1 Vbar1M)
    g_det  = real(fft2(Om1det)) dx^2 dy^2

linear in M, and Om1 / g exactly for M = 1.  Omega_det,s is the structure-factor sum of slice s with g_det, built the way Omega_s
is built from g, and the TDS generated in slice s that lands on the detector, for probe p, is

    w_s(r)  = 1 - exp(-2 sigma^2 Omega_det,s(r))
    I[p, d, s] = sum_r |psi_p,s(r)|^2 w_s(r)             psi_p,s = the wave arriving at slice s, before t_s

TDS electrons are not propagated further; the signal at thickness k is sum_{s <= k} I[p, d, s].  For a detector that covers the whole
plane w = 1 - |t|^2, so sum_r |psi_exit|^2 + sum_s I_s = sum_r |psi_0|^2 exactly (the propagator has unit modulus).

The device builds the same tables and sums itself (csrc/tds.h behind msl_set_tds).  The approximation inherits the heavy-atom limit
of the second cumulant (absorptive.py) and adds its own: the split of the absorbed intensity over the detectors is that of single
thermal scattering inside one slice, and what the TDS electrons do afterwards is left out.

Not built: the reduction fused into a pass kernel of the one-pass loop, segmented detectors and CoM signals, the propagation of the
TDS electrons, TDS on run_polar() / run_diffraction(), more than 4 detectors.
"""
from __future__ import annotations

import numpy as np

from .absorptive import debye_waller

MAX_TDS_DETECTORS = 4


def tds_tables(f, q2, u, dx, dy, M):
    """g_det of one species and one detector: f its form-factor table on the fftfreq grid, q2 = kx^2 + ky^2 there, u its rms width
    per axis, M the detector's membership there (bool or 0 / 1).  u = 0: zeros.  M = 1: absorptive_tables' g."""
    f = np.asarray(f, dtype=np.float64)
    M = np.asarray(M, dtype=np.float64)
    if M.shape != f.shape:
        raise ValueError(f"tds_tables: membership {M.shape} does not match the table {f.shape}")
    if float(u) == 0.0:
        return np.zeros(f.shape, dtype=np.float64)
    cell = float(dx) ** 2 * float(dy) ** 2
    D = debye_waller(q2, u)
    V1 = np.fft.ifft2(f).real / cell
    Vbar1 = np.fft.ifft2(f * D).real / cell
    V1M = np.fft.ifft2(M * f).real / cell
    Vbar1M = np.fft.ifft2(M * f * D).real / cell
    Om1det = 0.5 * (np.fft.ifft2(D * np.fft.fft2(V1 * V1M)).real - Vbar1 * Vbar1M)
    return np.fft.fft2(Om1det).real * cell


def tds_weight(Omega_det, sigma_e):
    """w = 1 - exp(-2 sigma^2 Omega_det), sigma_e the interaction constant"""
    return -np.expm1(-2.0 * float(sigma_e) ** 2 * np.asarray(Omega_det, dtype=np.float64))


def tds_signal(psi0, transmission, weight, propagator):
    """The float64 slice loop: psi0 (P, nx, ny) incident waves, transmission (nz, nx, ny) complex (absorptive_transmission of every
    slice), weight (D, nz, nx, ny) (tds_weight of every detector and slice), propagator (nx, ny) on the fftfreq grid (the Fresnel
    factor of one slice; tilt.tilted_propagator) -> (I (P, D, nz), exit waves (P, nx, ny))."""
    psi = np.array(psi0, dtype=np.complex128)
    if psi.ndim == 2:
        psi = psi[None]
    t = np.asarray(transmission)
    w = np.asarray(weight, dtype=np.float64)
    if t.ndim != 3 or t.shape[1:] != psi.shape[1:]:
        raise ValueError(f"tds_signal: transmission {t.shape} does not match the waves {psi.shape}: expected (nz, nx, ny)")
    if w.ndim != 4 or w.shape[1:] != t.shape:
        raise ValueError(f"tds_signal: weight {w.shape} does not match the transmission {t.shape}: expected (D, nz, nx, ny)")
    nz = t.shape[0]
    I = np.zeros((psi.shape[0], w.shape[0], nz), dtype=np.float64)
    for s in range(nz):
        I[:, :, s] = np.einsum("pxy,dxy->pd", np.abs(psi) ** 2, w[:, s])
        psi = t[s][None] * psi
        if s < nz - 1:
            psi = np.fft.ifft2(np.asarray(propagator)[None] * np.fft.fft2(psi, axes=(-2, -1)), axes=(-2, -1))
    return I, psi


def tds_members(detectors, nx, ny, dx, dy, wavelength):
    """(nx, ny) uint16 for msl_set_tds: bit d set where the fftfreq pixel lies in detector d"""
    from .stem_data import detector_bitmask
    return detector_bitmask(detectors, np.fft.fftfreq(nx, dx), np.fft.fftfreq(ny, dy), wavelength)


def check_tds_detectors(detectors):
    """the detectors of MultisliceCalculator(tds=True): at most 4 annuli that read the intensity (before any device work)"""
    if detectors is None:
        raise ValueError("tds=True needs detectors=[...]: the TDS signal is that of run_detectors()")
    if len(detectors) > MAX_TDS_DETECTORS:
        raise NotImplementedError(f"tds: more than {MAX_TDS_DETECTORS} detectors is not built (got {len(detectors)})")
    for d in detectors:
        if d.azimuth is not None:
            raise NotImplementedError(f"tds: a segmented detector ({d.name!r}, azimuth={d.azimuth}) is not built")
        if d.signal != "intensity":
            raise NotImplementedError(f"tds: the signal {d.signal!r} of detector {d.name!r} is not built (TDS adds to an intensity)")
