"""Polar detector: every exit spectrum of a scan summed into radial rings x azimuthal sectors
(MultisliceCalculator(polar=PolarDetector(...)).run_polar()).

detectors=[...] fixes at most 16 regions before the run; diffraction=Diffraction(...) keeps whole frame-averaged patterns on the
host.  The polar detector lies between them: R rings x A sectors, a few hundred to a few thousand numbers per probe position (and
frame), from which any annular, segmented or DPC detector whose edges are ring edges and sector boundaries is a sum of bins chosen
AFTER the run.  The HIP pass msl_polar_detect (pyslice_amd/csrc/polar.h) forms the bins on the device as soon as the slice loop has
written a probe batch, so a scan needs no (P, T, nx, ny) array.  This module is the definition, in NumPy: the bin of every stored
pixel (polar_bins, the rules of stem_data.Detector.member), the reference sums (polar_signals) and the result (PolarData).
"""
from __future__ import annotations

import math
from dataclasses import dataclass, replace
from typing import Any, Optional, Sequence

import numpy as np

from ._native import POLAR_MAX_BINS, POLAR_NONE
from .stem_data import Detector, STEMData, scan_axes, scan_image

EDGE_TOL = 1e-9        # mrad (degrees for sector boundaries): how close an angle of integrate() must be to an edge


@dataclass(frozen=True)
class PolarDetector:
    """The request: rings of width `step` from `inner` up to at least `outer` (mrad), each cut into n_azimuthal sectors whose first
    boundary lies at `rotation` degrees (phi = atan2(ky, kx), as Detector.azimuth).  R = ceil((outer - inner) / step) rings with the
    edges e_r = inner + r * step, r = 0 .. R: the last edge is inner + R * step, not outer.  Ring r holds e_r < theta <= e_{r+1}
    (ring 0 of inner = 0 also theta = 0: Detector's rule), sector a holds rotation + a * 360 / A <= phi < rotation + (a + 1) * 360 / A;
    the bin of a pixel is r * A + a.  per_frame=True keeps the signals of every frame, (P, T, R, A), instead of their mean."""
    outer: float
    step: float = 1.0
    inner: float = 0.0
    n_azimuthal: int = 1
    rotation: float = 0.0
    per_frame: bool = False

    def __post_init__(self):
        for name in ("outer", "step", "inner"):
            v = getattr(self, name)
            if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, float, np.integer, np.floating)) or not np.isfinite(v) or v < 0:
                raise ValueError(f"PolarDetector: {name} must be a finite angle >= 0 mrad, got {v!r}")
            object.__setattr__(self, name, float(v))
        if self.step <= 0:
            raise ValueError(f"PolarDetector: step must be > 0 mrad, got {self.step}")
        if self.outer <= self.inner:
            raise ValueError(f"PolarDetector: outer angle {self.outer} must exceed the inner angle {self.inner}")
        a = self.n_azimuthal
        if isinstance(a, (bool, np.bool_)) or not isinstance(a, (int, np.integer)) or a < 1:
            raise ValueError(f"PolarDetector: n_azimuthal must be an integer >= 1, got {a!r}")
        object.__setattr__(self, "n_azimuthal", int(a))
        rot = self.rotation
        if isinstance(rot, (bool, np.bool_)) or not isinstance(rot, (int, float, np.integer, np.floating)) or not np.isfinite(rot):
            raise ValueError(f"PolarDetector: rotation must be a finite angle in degrees, got {rot!r}")
        object.__setattr__(self, "rotation", float(rot))
        if not isinstance(self.per_frame, (bool, np.bool_)):
            raise ValueError(f"PolarDetector: per_frame must be True or False, got {self.per_frame!r}")
        object.__setattr__(self, "per_frame", bool(self.per_frame))
        if self.n_bins > POLAR_MAX_BINS:
            raise ValueError(f"PolarDetector: {self.n_rings} rings x {self.n_azimuthal} sectors = {self.n_bins} bins, at most "
                             f"{POLAR_MAX_BINS} (a larger step, or fewer sectors)")

    @property
    def n_rings(self) -> int:
        """R = ceil((outer - inner) / step); a quotient that float division leaves within EDGE_TOL mrad above a whole number of
        steps (1.1 / 0.1 = 11.000000000000002) counts as that whole number"""
        R = int(math.ceil((self.outer - self.inner) / self.step))
        if R > 1 and self.inner + (R - 1) * self.step >= self.outer - EDGE_TOL:
            R -= 1
        return R

    @property
    def n_bins(self) -> int:
        return self.n_rings * self.n_azimuthal

    @property
    def edges(self) -> np.ndarray:
        """(R + 1,) float64 ring edges in mrad"""
        return self.inner + np.arange(self.n_rings + 1, dtype=np.float64) * self.step


def polar_bins(polar: PolarDetector, kxs, kys, wavelength) -> np.ndarray:
    """(len(kxs), len(kys)) uint16: the bin r * A + a of every stored pixel, POLAR_NONE (0xFFFF) for a pixel in no bin.  q, phi and
    the edge radii are formed exactly as Detector.member forms them, so the union of the bins between two edges IS the member mask
    of the Detector with those edges."""
    kx = np.asarray(kxs, dtype=np.float32).astype(np.float64)
    ky = np.asarray(kys, dtype=np.float32).astype(np.float64)
    q = np.sqrt(kx[:, None] ** 2 + ky[None, :] ** 2)
    R, A = polar.n_rings, polar.n_azimuthal
    edges_q = (polar.edges * 1e-3) / wavelength
    ring = np.searchsorted(edges_q, q, side="left") - 1          # edge_r < q <= edge_{r+1}
    if polar.inner == 0:
        ring = np.where(q == 0, 0, ring)
    inside = (ring >= 0) & (ring < R)
    phi = np.degrees(np.arctan2(ky[None, :], kx[:, None])) % 360.0
    phi = np.where(phi >= 360.0, phi - 360.0, phi)
    sector = np.floor(((phi - polar.rotation) % 360.0) / (360.0 / A)).astype(np.int64)
    sector = np.clip(sector, 0, A - 1)
    return np.where(inside, ring * A + sector, POLAR_NONE).astype(np.uint16)


def bin_counts(bins, n_bins) -> np.ndarray:
    """(n_bins,) int64: the stored pixels of every bin"""
    b = np.asarray(bins).reshape(-1)
    return np.bincount(b[b != POLAR_NONE].astype(np.int64), minlength=int(n_bins)).astype(np.int64)


def polar_signals(W, bins, n_bins) -> np.ndarray:
    """W (..., wx, wy) complex -> (..., n_bins) float64: sum of |Psi|^2 over the pixels of each bin, in float64; an empty bin
    gives 0.  The reference of the device pass."""
    W = np.asarray(W)
    b = np.asarray(bins).reshape(-1)
    if W.shape[-2] * W.shape[-1] != b.size:
        raise ValueError(f"bin map of {b.size} pixels for spectra of {W.shape[-2]} x {W.shape[-1]}")
    lead = W.shape[:-2]
    I = np.abs(W.reshape(lead + (b.size,)).astype(np.complex128)) ** 2
    out = np.zeros(lead + (int(n_bins),), dtype=np.float64)
    order = np.argsort(b, kind="stable")
    order = order[: int((b != POLAR_NONE).sum())]                # (POLAR_NONE is the largest id: those pixels sort last)
    if order.size == 0:
        return out
    ids = b[order].astype(np.int64)
    if ids.max() >= int(n_bins):
        raise ValueError(f"bin id {ids.max()} in a map of {int(n_bins)} bins")
    starts = np.flatnonzero(np.r_[True, ids[1:] != ids[:-1]])
    out[..., ids[starts]] = np.add.reduceat(I[..., order], starts, axis=-1)
    return out


def _np(a):
    return a.detach().cpu().numpy() if hasattr(a, "detach") else np.asarray(a)


@dataclass
class PolarData:
    """Result of MultisliceCalculator.run_polar(): signals (P, R, A) float64 -- the mean over the frames of |Psi|^2 in ring r,
    sector a at probe p -- or (P, T, R, A) with PolarDetector(per_frame=True); the request `polar`; counts (R, A) int64, the stored
    pixels of every bin (0: an empty bin, whose signal is 0); edges (R + 1,) in mrad; the run's probe_positions / time / kxs / kys /
    probe, the scan axes xs / ys, and `stem`: the STEMData of the same pass when the run had detectors.
    With MultisliceCalculator(thickness=...) signals is (P, R, A, L) or (P, T, R, A, L): `layer` holds the slice indices of the L
    thickness entries, `thickness` the depth in Angstrom at the exit side of each slice, at(i) is the ordinary PolarData of entry i
    (its stem too), and integrate / image / profile / to_stem take layer=-1, the exit wave."""
    signals: np.ndarray
    polar: PolarDetector
    counts: np.ndarray
    edges: np.ndarray
    probe_positions: Any
    time: np.ndarray
    kxs: Any
    kys: Any
    probe: Any
    xs: np.ndarray = None
    ys: np.ndarray = None
    stem: Optional[STEMData] = None
    layer: Optional[np.ndarray] = None
    thickness: Optional[np.ndarray] = None
    tilts: Optional[list] = None            # the tilt.Tilt of every run of a precession average (tilt order); None otherwise
    coherence: Any = None                   # the coherence.Coherence of the run (None: a coherent probe)

    def source_blurred(self, sigma, periodic=True) -> "PolarData":
        """this result with the signals (and those of .stem) convolved over the scan with a Gaussian source of rms width sigma
        (Angstrom) per axis (coherence.blur_scan).  The probe positions must form a full regular raster (ValueError otherwise);
        periodic=True when the raster covers a periodic cell."""
        from .coherence import blur_positions
        return replace(self, signals=blur_positions(self.signals, self.probe_positions, sigma, periodic),
                       stem=None if self.stem is None else self.stem.source_blurred(sigma, periodic))

    def __post_init__(self):
        R, A = self.polar.n_rings, self.polar.n_azimuthal
        want = 4 if self.polar.per_frame else 3
        if self.layer is not None:
            if np.ndim(self.signals) != want + 1 or np.shape(self.signals)[-3:] != (R, A, len(self.layer)):
                raise ValueError(f"signals of shape {np.shape(self.signals)} for {R} rings x {A} sectors x {len(self.layer)} thickness entries"
                                 + (" per frame" if self.polar.per_frame else ""))
        elif np.ndim(self.signals) != want or np.shape(self.signals)[-2:] != (R, A):
            raise ValueError(f"signals of shape {np.shape(self.signals)} for {R} rings x {A} sectors"
                             + (" per frame" if self.polar.per_frame else ""))
        if self.xs is None or self.ys is None:
            self.xs, self.ys = scan_axes(self.probe_positions)

    def at(self, i: int) -> "PolarData":
        """the un-layered PolarData of thickness entry i (negative from the end: -1 is the exit wave)"""
        if self.layer is None:
            raise ValueError("this PolarData has no thickness axis: run with MultisliceCalculator(thickness=...)")
        from .thickness import entry
        j = entry(self.layer, i)
        return replace(self, signals=self.signals[..., j], layer=None, thickness=None,
                       stem=None if self.stem is None else self.stem.at(j))

    def poisson(self, dose, seed=None) -> np.ndarray:
        """uint32 of the shape of `signals`: the electrons every bin counts at `dose` (electrons per probe position, or a
        dose.Dose), drawn on the host by dose.poisson_counts from the signals per incident electron; probe p keyed by its index, the
        pixel index the row-major index of the rest (per_frame: every frame is an exposure of its own at that dose).  seed=None: the
        Dose's seed (0 for a number)."""
        from .dose import Dose, poisson_signals, probe_incident
        n_e = dose.electrons(self.probe_positions) if isinstance(dose, Dose) else dose
        if seed is None:
            seed = dose.seed if isinstance(dose, Dose) else 0
        return poisson_signals(self.signals, n_e, probe_incident(self.probe), seed)

    def _edge(self, what, angle) -> int:
        e = np.asarray(self.edges, dtype=np.float64)
        i = int(np.argmin(np.abs(e - angle)))
        if abs(e[i] - angle) > EDGE_TOL:
            j = int(np.clip(np.searchsorted(e, angle), 1, len(e) - 1))
            raise ValueError(f"{what}={angle} mrad is not a ring edge: the nearest edges are {e[j - 1]:g} and {e[j]:g} mrad")
        return i

    def _sectors(self, azimuth):
        A = self.polar.n_azimuthal
        if azimuth is None:
            return list(range(A))
        az = tuple(float(v) for v in azimuth)
        if len(az) != 2 or not all(0.0 <= v <= 360.0 for v in az) or az[0] == az[1]:
            raise ValueError(f"azimuth must be two different angles in [0, 360] degrees, got {azimuth}")
        width = 360.0 / A
        idx = []
        for v in az:
            x = ((v - self.polar.rotation) % 360.0) / width
            a = int(round(x))
            if abs(x - a) * width > EDGE_TOL:
                lo = (self.polar.rotation + math.floor(x) * width) % 360.0
                raise ValueError(f"azimuth {v} degrees is not a sector boundary: the nearest boundaries are {lo:g} and "
                                 f"{(lo + width) % 360.0:g} degrees")
            idx.append(a % A)
        a0, a1 = idx
        n = (a1 - a0) % A or A                                   # from boundary a0 round to boundary a1 (the whole circle: A sectors)
        return [(a0 + i) % A for i in range(n)]

    def integrate(self, inner=0.0, outer=None, azimuth=None, layer=-1) -> np.ndarray:
        """(P,) -- (P, T) per frame: the sum of the bins between the ring edges `inner` and `outer` (None: the last edge) and, with
        azimuth=(phi0, phi1), of the sectors phi0 <= phi < phi1 (wrapping through 0 when phi0 > phi1, as Detector.azimuth): the
        intensity signal of Detector(inner=inner, outer=outer, azimuth=azimuth).  ValueError when an angle is not an edge within
        1e-9 mrad, or not a sector boundary.  Of thickness entry `layer` when there is a thickness axis."""
        if self.layer is not None:
            return self.at(layer).integrate(inner, outer, azimuth)
        r0 = self._edge("inner", float(inner))
        r1 = len(self.edges) - 1 if outer is None else self._edge("outer", float(outer))
        if r1 <= r0:
            raise ValueError(f"outer angle {outer} must exceed the inner angle {inner}")
        return self.signals[..., r0:r1, :][..., self._sectors(azimuth)].sum(axis=(-2, -1))

    def image(self, inner=0.0, outer=None, azimuth=None, frames=None, layer=-1) -> np.ndarray:
        """(len(xs), len(ys)) scan image of integrate(inner, outer, azimuth): the mean over the frames (per_frame: all, or an index /
        slice / list of frame indices), every scan point taking its nearest probe's value (stem_data.scan_image)"""
        if self.layer is not None:
            return self.at(layer).image(inner, outer, azimuth, frames)
        s = self.integrate(inner, outer, azimuth)
        if self.polar.per_frame:
            if frames is not None:
                s = s[:, frames]
                if s.ndim == 1:
                    s = s[:, None]
            s = s.mean(axis=1)
        elif frames is not None:
            raise ValueError("frames: this PolarData holds the frame mean only (run with PolarDetector(per_frame=True))")
        return scan_image(s, self.probe_positions, self.xs, self.ys)

    def profile(self, probe_index=None, layer=-1) -> np.ndarray:
        """(R,): the radial profile -- summed over the sectors, averaged over the frames -- of one probe, or the mean over all"""
        if self.layer is not None:
            return self.at(layer).profile(probe_index)
        s = self.signals.sum(axis=-1)
        if self.polar.per_frame:
            s = s.mean(axis=1)
        return s.mean(axis=0) if probe_index is None else s[int(probe_index)]

    def to_stem(self, detectors: Sequence[Detector], layer=-1) -> STEMData:
        """STEMData of intensity detectors whose edges are ring edges and sector boundaries, chosen after the run: signals
        (P, T, D), so STEMData.image() and everything built on it applies.  Needs per_frame=True."""
        if self.layer is not None:
            return self.at(layer).to_stem(detectors)
        if not self.polar.per_frame:
            raise ValueError("to_stem() needs the signals of every frame: run with PolarDetector(per_frame=True)")
        dets = list(detectors)
        cols = []
        for d in dets:
            if not isinstance(d, Detector):
                raise ValueError(f"expected Detector objects, got {d!r}")
            if d.signal != "intensity":
                raise ValueError(f"detector {d.name!r}: polar bins hold |Psi|^2 only, signal {d.signal!r} cannot be formed from them")
            if d.outer is None:
                raise ValueError(f"detector {d.name!r} has no outer edge: the polar bins end at {self.edges[-1]:g} mrad (give outer=)")
            cols.append(self.integrate(d.inner, d.outer, d.azimuth))
        return STEMData(signals=np.stack(cols, axis=-1), detectors=dets, probe_positions=self.probe_positions, time=self.time,
                        kxs=self.kxs, kys=self.kys, probe=self.probe, xs=self.xs, ys=self.ys)
